"""ctypes binding of libqadc_hip.so (the C-ABI in include/qadc.h) for tests and bench.py.

Thin by design: numpy in, numpy out, no computation here.  Loading fails loudly when the HIP
library has not been built; there is no CPU fallback anywhere on this path.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "libqadc_hip.so")
if os.environ.get("QADC_TEST_HOOKS") == "1" and os.environ.get("QADC_LIB_PATH"):   # same-box A/B of two builds (tools/)
    LIB_PATH = os.environ["QADC_LIB_PATH"]

u8p = C.POINTER(C.c_uint8)
i8p = C.POINTER(C.c_int8)
u32p = C.POINTER(C.c_uint32)
i32p = C.POINTER(C.c_int32)
u64p = C.POINTER(C.c_uint64)
f32p = C.POINTER(C.c_float)

# every symbol include/qadc.h declares
SYMBOLS = [
    "qadc_last_error", "qadc_version", "qadc_index_create", "qadc_index_destroy",
    "qadc_index_add_partitions", "qadc_index_add_partition_interleaved",
    "qadc_index_add_partition_device", "qadc_index_add_partition_synthetic",
    "qadc_index_add_partition_shard", "qadc_index_add_partition_synthetic_shard", "qadc_query_scan_collect_candidates",
    "qadc_index_set_key_base", "qadc_index_finalize", "qadc_index_partition_count",
    "qadc_index_partition_size", "qadc_index_start_size", "qadc_set_option", "qadc_option_names",
    "qadc_index_read_codes", "qadc_query_scan", "qadc_query_scan_candidates", "qadc_scan_i8",
    "qadc_scan_i8_candidates", "qadc_scan_start", "qadc_query_scan_submit", "qadc_prescan_submit",
    "qadc_prescan_collect", "qadc_query_scan_submit_prescanned",
    "qadc_query_scan_collect", "qadc_index_set_pq", "qadc_index_set_rotation", "qadc_index_set_coarse", "qadc_search", "qadc_search_submit",
    "qadc_search_collect", "qadc_device_prepare", "qadc_stream_probe", "qadc_stream_layout", "qadc_pq_encode", "qadc_pq_encode_host", "qadc_ivf_encode_host", "qadc_pq_encode_mode", "qadc_pq_encode_host_mode", "qadc_ivf_encode_host_mode", "qadc_kmeans_iterations_host", "qadc_coarse_assign_host", "qadc_kmeans_iterations_host_mode", "qadc_replay_i8", "qadc_sort_keys_i8", "qadc_merge_streams_i8", "qadc_candidates_i8", "qadc_float_top1", "qadc_profile_read", "qadc_profile_reset", "qadc_index_set_split", "qadc_index_set_split6", "qadc_index_set_split5", "qadc_index_set_split_nib", "qadc_nib_choice", "qadc_index_set_split_bkt", "qadc_bkt_choice", "qadc_index_bkt_info", "qadc_index_bkt_read", "qadc_index_set_split_bkt_wide", "qadc_index_set_bkt_prune", "qadc_index_set_bkt_prune_lanes", "qadc_index_set_bkt_tiles", "qadc_bktw_choice", "qadc_index_bktw_info", "qadc_index_bktw_read",
    "qadc_dist_unique_id", "qadc_dist_init", "qadc_dist_collect", "qadc_dist_shutdown", "qadc_dist_merge_blocks", "qadc_dist_merge_blocks_host",
    "qadc_dist_init_transport", "qadc_dist_init_loopback", "qadc_shm_transport_open", "qadc_shm_transport_allgather", "qadc_shm_transport_allgather_host",
    "qadc_shm_transport_close", "qadc_shm_transport_error", "qadc_slot_assign", "qadc_slot_qtables", "qadc_place_partitions",
    "qadc_adc_index_create", "qadc_adc_index_destroy", "qadc_adc_index_add_partitions", "qadc_adc_index_partition_count",
    "qadc_adc_index_partition_size", "qadc_adc_query_scan", "qadc_adc_query_scan_candidates", "qadc_adc_index_reruns",
    "qadc_adc_index_set_pq", "qadc_adc_index_set_rotation", "qadc_adc_index_set_coarse", "qadc_adc_index_set_table_budget",
    "qadc_adc_search", "qadc_adc_search_candidates", "qadc_adc_search_tables", "qadc_adc_encode_host",
    "qadc_adc_index_set_finish", "qadc_adc_index_host_finishes", "qadc_adc_search_device", "qadc_adc_query_scan_device",
    "qadc_adc_index_create_view", "qadc_adc_index_create16", "qadc_adc_encode16_host",
    "qadc_adc_index_add_vectors", "qadc_adc_index_add_vectors_device", "qadc_adc_index_read_partition", "qadc_adc_index_reserve",
    "qadc_adc_index_relocations",
    "qadc_adc_index_add_vectors_labelled", "qadc_adc_index_add_vectors_labelled_device",
    "qadc_index_add_vectors_labelled", "qadc_index_add_vectors_labelled_device",
    "qadc_index_add_vectors", "qadc_index_add_vectors_device", "qadc_index_read_partition", "qadc_index_reserve",
    "qadc_index_relocations",
    "qadc_adc_index_remove_labels", "qadc_adc_index_remove_labels_device", "qadc_index_remove_labels", "qadc_index_remove_labels_device",
    "qadc_pq_train_host", "qadc_pq_train_device",
    "qadc_pq_train16_host", "qadc_pq_train16_device", "qadc_pq_update16_host",
    "qadc_opq_cross_host", "qadc_opq_cross_device", "qadc_procrustes_host", "qadc_opq_train_host", "qadc_opq_train_device",
    "qadc_kmeans_seed_host", "qadc_kmeans_seed_device",
    "qadc_pq_repair_host", "qadc_pq_train_repair_host", "qadc_pq_train_repair_device", "qadc_pq_train16_repair_host",
    "qadc_pq_train16_repair_device", "qadc_opq_train_repair_host", "qadc_opq_train_repair_device",
    "qadc_adc_filter_create", "qadc_adc_filter_create_device", "qadc_adc_filter_info", "qadc_adc_filter_destroy", "qadc_adc_index_set_filter",
    "qadc_adc_query_scan_filtered", "qadc_adc_query_scan_device_filtered", "qadc_adc_query_scan_candidates_filtered",
    "qadc_adc_search_filtered", "qadc_adc_search_device_filtered", "qadc_adc_search_candidates_filtered",
    "qadc_refine_create", "qadc_refine_destroy", "qadc_refine_add", "qadc_refine_add_device", "qadc_refine_reserve", "qadc_refine_info",
    "qadc_refine_relocations", "qadc_refine_rerank", "qadc_refine_rerank_device",
    "qadc_refine_create_keyed", "qadc_refine_put", "qadc_refine_put_device", "qadc_refine_remove", "qadc_refine_remove_device",
    "qadc_refine_keyed_info", "qadc_refine_keyed_slot",
    "qadc_refine_knn", "qadc_refine_knn_device", "qadc_refine_set_knn_plan",
    "qadc_refine_knn_probed", "qadc_refine_knn_probed_device", "qadc_adc_index_assign", "qadc_adc_index_assign_device",
    "qadc_adc_search_exact", "qadc_adc_search_exact_device",
    "qadc_refine_create_sq8", "qadc_refine_sq_range_host", "qadc_refine_sq_range_device", "qadc_refine_sq_info", "qadc_refine_get",
    "qadc_refine_get_device",
    "qadc_pq_decode_host", "qadc_pq_decode_device", "qadc_adc_index_reconstruct", "qadc_adc_index_reconstruct_device",
    "qadc_adc_index_reconstruct_rows", "qadc_adc_index_reconstruct_rows_device",
    "qadc_adc_range_scan", "qadc_adc_range_scan_device", "qadc_adc_range_search", "qadc_adc_range_search_device",
    "qadc_adc_range_collect", "qadc_adc_range_collect_device",
    "qadc_refine_range", "qadc_refine_range_device", "qadc_refine_rerank_range", "qadc_refine_rerank_range_device",
    "qadc_refine_range_collect", "qadc_refine_range_collect_device", "qadc_refine_set_range_plan", "qadc_refine_range_reruns",
    "qadc_refine_set_metric", "qadc_refine_metric",
]


class Profile(C.Structure):
    _fields_ = [("scan_launches", C.c_uint64), ("scan_codes", C.c_uint64), ("scan_ms", C.c_double),
                ("small_launches", C.c_uint64), ("small_codes", C.c_uint64), ("small_ms", C.c_double),
                ("start_codes", C.c_uint64), ("start_ms", C.c_double), ("candidates", C.c_uint64),
                ("regrows", C.c_uint64), ("host_replay_ms", C.c_double), ("host_plan_ms", C.c_double),
                ("host_heap_ms", C.c_double), ("host_sorted_queries", C.c_uint64), ("mq_launches", C.c_uint64),
                ("pass_codes", C.c_uint64), ("wgq_launches", C.c_uint64), ("wgq_queries", C.c_uint64),
                ("wgq_codes", C.c_uint64), ("wgq_ms", C.c_double), ("wgq_front_cycles", C.c_uint64),
                ("wgq_scan_cycles", C.c_uint64), ("wgq_sort_cycles", C.c_uint64), ("head_launches", C.c_uint64),
                ("group_launches", C.c_uint64), ("group_fallbacks", C.c_uint64),
                ("group_head_ms", C.c_double), ("group_scan_ms", C.c_double), ("group_order_ms", C.c_double),
                ("group_head_codes", C.c_uint64), ("group_pairs", C.c_uint64), ("group_seats", C.c_uint64),
                ("group_pass_codes8", C.c_uint64), ("group_pass_codes4", C.c_uint64), ("group_batches", C.c_uint64),
                ("front_sharded_batches", C.c_uint64), ("dist_async_collects", C.c_uint64),
                ("lone_front_launches", C.c_uint64), ("split_launches", C.c_uint64), ("split_codes", C.c_uint64),
                ("split_copy_bytes", C.c_uint64), ("split_copy_failed", C.c_uint64),
                ("split6_launches", C.c_uint64), ("split6_codes", C.c_uint64), ("split_survivors", C.c_uint64),
                ("split5_launches", C.c_uint64), ("split5_codes", C.c_uint64), ("split5_survivors", C.c_uint64),
                ("nib_copy_bytes", C.c_uint64), ("nib_copy_failed", C.c_uint64),
                ("nib_launches", C.c_uint64), ("nib_codes", C.c_uint64), ("nib_survivors", C.c_uint64),
                ("nib8_launches", C.c_uint64), ("nib8_codes", C.c_uint64), ("nib8_survivors", C.c_uint64),
                ("bkt_copy_bytes", C.c_uint64), ("bkt_copy_slots", C.c_uint64), ("bkt_copy_failed", C.c_uint64),
                ("bkt_copy_padded_out", C.c_uint64), ("bkt_launches", C.c_uint64), ("bkt_codes", C.c_uint64),
                ("bkt_slots", C.c_uint64), ("bkt_survivors", C.c_uint64),
                ("bkt4_launches", C.c_uint64), ("bkt5_launches", C.c_uint64), ("bkt6_launches", C.c_uint64),
                ("bkt7_launches", C.c_uint64),
                ("bktw_copy_bytes", C.c_uint64), ("bktw_copy_slots", C.c_uint64), ("bktw_copy_fallback", C.c_uint64),
                ("bktw_launches", C.c_uint64), ("bktw_codes", C.c_uint64), ("bktw_slots", C.c_uint64),
                ("bktw_survivors", C.c_uint64), ("bktw3_launches", C.c_uint64), ("bktw4_launches", C.c_uint64),
                ("bktw5_launches", C.c_uint64), ("bktw6_launches", C.c_uint64),
                ("bktw_prune_skipped", C.c_uint64), ("bktw_prune_run", C.c_uint64), ("bktw_prune_groups", C.c_uint64),
                ("bktw_prune_quarters", C.c_uint64)]


QADC_E_ARG, QADC_E_HIP, QADC_E_CAPACITY, QADC_E_STATE = -1, -2, -3, -4   # include/qadc.h
QADC_ADC_ENCODE16_CHUNK = 262144   # include/qadc.h: vectors qadc_adc_encode16_host encodes per pass
QADC_ADC_ADD_CHUNK = 262144        # include/qadc.h: vectors qadc_adc_index_add_vectors encodes and appends per pass
QADC_INDEX_ADD_CHUNK = 262144      # ... and qadc_index_add_vectors
ADC_RANGE_SORT_LDS = 4096          # include/qadc.h QADC_ADC_RANGE_SORT_LDS: rows of a range query sorted in LDS; more take radix passes


class QadcError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise QadcError("libqadc_hip.so is not built (run __graft_entry__.build() or make -C quick-adc_amd); "
                            "the Quick-ADC engine has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.qadc_last_error.restype = C.c_char_p
        L.qadc_version.restype = C.c_char_p
        L.qadc_index_partition_size.restype = C.c_uint32
        L.qadc_index_start_size.restype = C.c_uint32
        L.qadc_index_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int]
        L.qadc_index_destroy.argtypes = [C.c_void_p]
        L.qadc_index_add_partitions.argtypes = [C.c_void_p, C.c_int, C.POINTER(u8p), C.POINTER(u32p), u32p]
        L.qadc_index_add_partition_interleaved.argtypes = [C.c_void_p, u8p, u32p, C.c_uint32]
        L.qadc_index_add_partition_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.qadc_index_add_partition_synthetic.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64]
        L.qadc_index_add_partition_shard.argtypes = [C.c_void_p, u8p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, u8p,
                                                     C.c_uint32]
        L.qadc_index_add_partition_synthetic_shard.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                               C.c_uint64, C.c_uint32]
        L.qadc_query_scan_collect_candidates.argtypes = [C.c_void_p, C.c_int, C.c_uint64, u32p, i8p, C.POINTER(C.c_uint16),
                                                         u64p, i32p, f32p, f32p]
        L.qadc_index_set_key_base.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
        L.qadc_index_finalize.argtypes = [C.c_void_p, C.c_float]
        L.qadc_index_partition_count.argtypes = [C.c_void_p]
        L.qadc_index_partition_size.argtypes = [C.c_void_p, C.c_int]
        L.qadc_index_start_size.argtypes = [C.c_void_p, C.c_int]
        L.qadc_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        L.qadc_index_set_split.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
        L.qadc_index_set_split6.argtypes = [C.c_void_p, C.c_uint64]
        L.qadc_index_set_split5.argtypes = [C.c_void_p, C.c_uint64]
        L.qadc_index_set_split_nib.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int]
        L.qadc_nib_choice.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.qadc_index_set_split_bkt.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double]
        L.qadc_bkt_choice.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.qadc_index_bkt_info.argtypes = [C.c_void_p, C.c_int, u64p, u64p, u64p]
        L.qadc_index_bkt_read.argtypes = [C.c_void_p, C.c_int, u64p, u8p, u8p]
        L.qadc_index_set_split_bkt_wide.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double]
        L.qadc_index_set_bkt_prune.argtypes = [C.c_void_p, C.c_int]
        L.qadc_index_set_bkt_prune_lanes.argtypes = [C.c_void_p, C.c_int]
        L.qadc_index_set_bkt_tiles.argtypes = [C.c_void_p, C.c_int]
        L.qadc_bktw_choice.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.qadc_index_bktw_info.argtypes = [C.c_void_p, C.c_int, u64p, u64p, u64p]
        L.qadc_index_bktw_read.argtypes = [C.c_void_p, C.c_int, u64p, u8p, u8p]
        L.qadc_index_read_codes.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, u8p]
        L.qadc_query_scan.argtypes = [C.c_void_p, C.c_int, C.c_int, i32p, f32p, C.c_int, u32p, i8p, i32p, i32p,
                                      f32p, f32p, i8p]
        L.qadc_query_scan_candidates.argtypes = [C.c_void_p, C.c_int, C.c_int, i32p, f32p, C.c_int, C.c_uint64,
                                                 u32p, i8p, u64p, i32p, f32p, f32p]
        L.qadc_scan_i8.argtypes = [C.c_void_p, C.c_int, C.c_int, i32p, i8p, C.c_int, u32p, i8p, i32p]
        L.qadc_scan_i8_candidates.argtypes = [C.c_void_p, C.c_int, C.c_int, i32p, i8p, C.c_int, C.c_uint64,
                                              u32p, i8p, u64p]
        L.qadc_scan_start.argtypes = [C.c_void_p, C.c_int, C.c_int, i32p, f32p, C.c_int, f32p]
        L.qadc_query_scan_submit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, i32p, f32p, C.c_int]
        L.qadc_prescan_submit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, i32p, f32p, C.c_int, C.c_int, C.c_int]
        L.qadc_prescan_collect.argtypes = [C.c_void_p, C.c_int, f32p]
        L.qadc_query_scan_submit_prescanned.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, i32p, f32p, C.c_int,
                                                        f32p, C.c_int]
        L.qadc_query_scan_collect.argtypes = [C.c_void_p, C.c_int, u32p, i8p, i32p, i32p, f32p, f32p, i8p]
        L.qadc_index_set_pq.argtypes = [C.c_void_p, C.c_int, f32p]
        L.qadc_index_set_rotation.argtypes = [C.c_void_p, f32p]
        L.qadc_index_set_coarse.argtypes = [C.c_void_p, C.c_int, f32p]
        L.qadc_search.argtypes = [C.c_void_p, C.c_int, f32p, C.c_int, C.c_int, u32p, i8p, i32p, i32p, i32p]
        L.qadc_search_submit.argtypes = [C.c_void_p, C.c_int, C.c_int, f32p, C.c_int, C.c_int]
        L.qadc_search_collect.argtypes = [C.c_void_p, C.c_int, u32p, i8p, i32p, i32p, i32p]
        L.qadc_pq_encode.argtypes = [C.c_int, C.c_int, f32p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
        L.qadc_pq_encode_host.argtypes = [C.c_int, C.c_int, f32p, f32p, C.c_uint64, u8p, C.c_int]
        L.qadc_ivf_encode_host.argtypes = [C.c_int, C.c_int, f32p, f32p, C.c_int, f32p, f32p, C.c_uint64, i32p, u8p, C.c_int]
        L.qadc_pq_encode_mode.argtypes = [C.c_int, C.c_int, f32p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.qadc_pq_encode_host_mode.argtypes = [C.c_int, C.c_int, f32p, f32p, C.c_uint64, u8p, C.c_int, C.c_int, C.c_int]
        L.qadc_ivf_encode_host_mode.argtypes = [C.c_int, C.c_int, f32p, f32p, C.c_int, f32p, f32p, C.c_uint64, i32p, u8p, C.c_int, C.c_int,
                                                C.c_int]
        L.qadc_kmeans_iterations_host.argtypes = [f32p, C.c_uint64, C.c_int, C.c_int, f32p, C.c_int, i32p, C.c_int]
        L.qadc_coarse_assign_host.argtypes = [f32p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, i32p, C.c_int]
        L.qadc_kmeans_iterations_host_mode.argtypes = [f32p, C.c_uint64, C.c_int, C.c_int, f32p, C.c_int, i32p, C.c_int, C.c_int]
        L.qadc_replay_i8.argtypes = [C.c_uint64, u32p, i8p, C.c_int, C.c_int, u32p, i8p, i32p]
        L.qadc_sort_keys_i8.argtypes = [C.c_int, u32p, i8p, u32p]
        L.qadc_merge_streams_i8.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, i32p, C.c_uint64, C.c_int,
                                            C.c_int, i32p, u32p, i8p, i32p]
        L.qadc_candidates_i8.argtypes = [C.c_void_p, C.c_int, i8p, i8p]
        L.qadc_float_top1.argtypes = [C.c_void_p, C.c_int, f32p, u32p, u32p, f32p]
        L.qadc_dist_unique_id.argtypes = [u8p]
        L.qadc_dist_init.argtypes = [C.c_void_p, C.c_int, C.c_int, u8p]
        L.qadc_dist_collect.argtypes = [C.c_void_p, C.c_int, u32p, i8p, i32p, i32p, f32p, C.c_int, f32p]
        L.qadc_dist_shutdown.argtypes = [C.c_void_p]
        L.qadc_dist_merge_blocks.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, u64p, C.c_uint64, u32p, i8p, i32p]
        L.qadc_dist_merge_blocks_host.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, u64p, C.c_uint64, u32p, i8p, i32p]
        L.qadc_dist_init_transport.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.qadc_dist_init_loopback.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.qadc_shm_transport_open.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_uint64, C.c_double, C.POINTER(C.c_void_p)]
        L.qadc_shm_transport_allgather.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.qadc_shm_transport_allgather_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.qadc_shm_transport_close.argtypes = [C.c_void_p]
        L.qadc_shm_transport_error.restype = C.c_char_p
        L.qadc_slot_assign.argtypes = [C.c_void_p, C.c_int, i32p]
        L.qadc_slot_qtables.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, i8p]
        L.qadc_place_partitions.argtypes = [C.c_int, u32p, C.c_int, i32p]
        L.qadc_profile_read.argtypes = [C.c_void_p, C.POINTER(Profile)]
        L.qadc_profile_reset.argtypes = [C.c_void_p]
        L.qadc_adc_index_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int]
        L.qadc_adc_index_destroy.argtypes = [C.c_void_p]
        L.qadc_adc_index_create_view.argtypes = [C.POINTER(C.c_void_p), C.c_void_p]
        L.qadc_adc_index_create16.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int]
        L.qadc_adc_index_add_partitions.argtypes = [C.c_void_p, C.c_int, C.POINTER(u8p), C.POINTER(u32p), u32p]
        L.qadc_adc_index_partition_count.argtypes = [C.c_void_p]
        L.qadc_adc_index_partition_size.argtypes = [C.c_void_p, C.c_int]
        L.qadc_adc_index_partition_size.restype = C.c_uint32
        L.qadc_adc_index_reruns.argtypes = [C.c_void_p]
        L.qadc_adc_index_reruns.restype = C.c_uint64
        L.qadc_adc_index_set_pq.argtypes = [C.c_void_p, C.c_int, f32p]
        L.qadc_adc_index_set_rotation.argtypes = [C.c_void_p, f32p]
        L.qadc_adc_index_set_coarse.argtypes = [C.c_void_p, C.c_int, f32p]
        L.qadc_adc_index_set_table_budget.argtypes = [C.c_void_p, C.c_uint64]
        L.qadc_adc_search.argtypes = [C.c_void_p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_int, u32p, f32p, i32p, i32p]
        L.qadc_adc_search_candidates.argtypes = [C.c_void_p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, u32p, f32p,
                                                 u64p, i32p]
        L.qadc_adc_search_tables.argtypes = [C.c_void_p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, i32p, f32p]
        L.qadc_adc_encode_host.argtypes = [C.c_int, C.c_int, f32p, f32p, C.c_int, f32p, f32p, C.c_uint64, C.c_int, i32p, u8p, C.c_int]
        L.qadc_adc_encode16_host.argtypes = L.qadc_adc_encode_host.argtypes
        L.qadc_adc_query_scan.argtypes = [C.c_void_p, C.c_int, C.c_int, i32p, f32p, C.c_int, C.c_int, u32p, f32p, i32p]
        L.qadc_adc_query_scan_candidates.argtypes = [C.c_void_p, C.c_int, C.c_int, i32p, f32p, C.c_int, C.c_int, C.c_uint64,
                                                     u32p, f32p, u64p]
        L.qadc_adc_index_set_finish.argtypes = [C.c_void_p, C.c_int]
        L.qadc_adc_index_host_finishes.argtypes = [C.c_void_p]
        L.qadc_adc_index_host_finishes.restype = C.c_uint64
        L.qadc_adc_search_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p]
        L.qadc_adc_query_scan_device.argtypes = [C.c_void_p, C.c_int, C.c_int, i32p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]
        L.qadc_adc_index_add_vectors.argtypes = [C.c_void_p, f32p, C.c_uint64, C.c_uint32, C.c_int]
        L.qadc_adc_index_add_vectors_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int]
        L.qadc_adc_index_read_partition.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, u8p, u32p]
        L.qadc_adc_index_reserve.argtypes = [C.c_void_p, C.c_int, u32p]
        L.qadc_adc_index_relocations.argtypes = [C.c_void_p]
        L.qadc_adc_index_relocations.restype = C.c_uint64
        L.qadc_index_add_vectors.argtypes = [C.c_void_p, f32p, C.c_uint64, C.c_uint32, C.c_int]
        L.qadc_adc_index_add_vectors_labelled.argtypes = [C.c_void_p, f32p, u32p, C.c_uint64, C.c_int]
        L.qadc_adc_index_add_vectors_labelled_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
        L.qadc_index_add_vectors_labelled.argtypes = [C.c_void_p, f32p, u32p, C.c_uint64, C.c_int]
        L.qadc_index_add_vectors_labelled_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
        L.qadc_index_add_vectors_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int]
        L.qadc_index_read_partition.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, u8p, u32p]
        L.qadc_index_reserve.argtypes = [C.c_void_p, C.c_int, u32p]
        L.qadc_index_relocations.argtypes = [C.c_void_p]
        L.qadc_index_relocations.restype = C.c_uint64
        L.qadc_pq_train_host.argtypes = [f32p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, C.c_int, C.c_void_p, u64p,
                                         C.c_int, C.c_int, C.c_int]
        L.qadc_pq_train_device.argtypes = [C.c_void_p] + L.qadc_pq_train_host.argtypes[1:]
        L.qadc_pq_train16_host.argtypes = [f32p, C.c_uint64, C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, C.c_int, C.c_void_p, u64p,
                                           C.c_int, C.c_int, C.c_int]
        L.qadc_pq_train16_device.argtypes = [C.c_void_p] + L.qadc_pq_train16_host.argtypes[1:]
        L.qadc_pq_update16_host.argtypes = [f32p, C.c_uint64, C.c_int, C.c_int, C.c_void_p, f32p, u32p, C.c_int, C.c_int]
        f64p = C.POINTER(C.c_double)
        L.qadc_opq_cross_host.argtypes = [f32p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p, f32p, f64p, C.c_int, C.c_int]
        L.qadc_opq_cross_device.argtypes = [C.c_void_p] + L.qadc_opq_cross_host.argtypes[1:]
        L.qadc_procrustes_host.argtypes = [f64p, C.c_int, f32p, i32p]
        L.qadc_opq_train_host.argtypes = [f32p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, C.c_int, C.c_int, C.c_void_p,
                                          u64p, i32p, C.c_int, C.c_int, C.c_int]
        L.qadc_opq_train_device.argtypes = [C.c_void_p] + L.qadc_opq_train_host.argtypes[1:]
        L.qadc_kmeans_seed_host.argtypes = [f32p, C.c_uint64, C.c_int, C.c_int, C.c_int64, C.c_int, f32p, f32p, C.c_uint64, f32p, u32p, u64p,
                                            C.c_int]
        L.qadc_kmeans_seed_device.argtypes = [C.c_void_p] + L.qadc_kmeans_seed_host.argtypes[1:]
        L.qadc_pq_repair_host.argtypes = [f32p, C.c_uint64, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p, u32p, C.c_int]
        for name in ("qadc_pq_train", "qadc_pq_train16", "qadc_opq_train"):    # ..., sum_mode, repair, repaired_out, device_id
            for form in ("_host", "_device"):
                old = getattr(L, name + form).argtypes
                getattr(L, name + "_repair" + form).argtypes = old[:-1] + [C.c_int, u64p, C.c_int]
        for name in ("qadc_adc_index_remove_labels", "qadc_index_remove_labels"):
            getattr(L, name).argtypes = [C.c_void_p, u32p, C.c_uint64, u64p]
            getattr(L, name + "_device").argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, u64p]
        L.qadc_adc_filter_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, u32p, C.c_uint64, C.c_int]
        L.qadc_adc_filter_create_device.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_uint64, C.c_int]
        L.qadc_adc_filter_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), u32p, u32p, u64p]
        L.qadc_adc_filter_destroy.argtypes = [C.c_void_p]
        L.qadc_adc_index_set_filter.argtypes = [C.c_void_p, C.c_void_p]
        for name in ("qadc_adc_query_scan", "qadc_adc_query_scan_device", "qadc_adc_query_scan_candidates", "qadc_adc_search",
                     "qadc_adc_search_device", "qadc_adc_search_candidates"):   # the plain form's arguments, then filters [nq]
            getattr(L, name + "_filtered").argtypes = getattr(L, name).argtypes + [C.POINTER(C.c_void_p)]
        filt = C.POINTER(C.c_void_p)
        L.qadc_adc_range_scan.argtypes = [C.c_void_p, C.c_int, C.c_int, i32p, f32p, f32p, C.c_int, filt, u64p]
        L.qadc_adc_range_scan_device.argtypes = [C.c_void_p, C.c_int, C.c_int, i32p, C.c_void_p, f32p, C.c_int, filt, u64p]
        L.qadc_adc_range_search.argtypes = [C.c_void_p, C.c_int, f32p, C.c_int, f32p, C.c_int, C.c_int, filt, i32p, u64p]
        L.qadc_adc_range_search_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, f32p, C.c_int, C.c_int, filt, i32p, u64p]
        L.qadc_adc_range_collect.argtypes = [C.c_void_p, C.c_uint64, u32p, f32p]
        L.qadc_adc_range_collect_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.qadc_refine_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int]
        L.qadc_refine_destroy.argtypes = [C.c_void_p]
        L.qadc_refine_create_keyed.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int]
        L.qadc_refine_put.argtypes = [C.c_void_p, f32p, u32p, C.c_uint64]
        L.qadc_refine_put_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.qadc_refine_remove.argtypes = [C.c_void_p, u32p, C.c_uint64, u64p]
        L.qadc_refine_remove_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, u64p]
        L.qadc_refine_keyed_info.argtypes = [C.c_void_p, u64p, u64p, u64p, u64p, u64p, u64p]
        L.qadc_refine_keyed_slot.argtypes = [C.c_uint32, C.c_int]
        L.qadc_refine_keyed_slot.restype = C.c_uint32
        L.qadc_refine_add.argtypes = [C.c_void_p, f32p, C.c_uint64, C.c_uint32]
        L.qadc_refine_add_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
        L.qadc_refine_reserve.argtypes = [C.c_void_p, C.c_uint64]
        L.qadc_refine_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), u32p, u64p, u64p]
        L.qadc_refine_relocations.argtypes = [C.c_void_p]
        L.qadc_refine_relocations.restype = C.c_uint64
        L.qadc_refine_rerank.argtypes = [C.c_void_p, C.c_int, f32p, C.c_int, u32p, i32p, f32p, C.c_int, u32p, f32p, i32p, u64p]
        L.qadc_refine_rerank_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p, u64p]
        L.qadc_refine_knn.argtypes = [C.c_void_p, C.c_int, f32p, C.c_int, C.c_void_p, u32p, f32p, i32p]
        L.qadc_refine_knn_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.qadc_refine_set_knn_plan.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
        L.qadc_refine_set_metric.argtypes = [C.c_void_p, C.c_int]
        L.qadc_refine_metric.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.qadc_refine_knn_probed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, f32p, C.c_int, i32p, C.c_int, C.c_void_p, u32p, f32p, i32p,
                                             C.POINTER(C.c_uint64)]
        L.qadc_refine_knn_probed_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.qadc_adc_index_assign.argtypes = [C.c_void_p, C.c_int, f32p, C.c_int, C.c_int, i32p]
        L.qadc_adc_index_assign_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.qadc_adc_search_exact.argtypes = [C.c_void_p, C.c_void_p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_void_p, u32p, f32p, i32p,
                                            C.POINTER(C.c_uint64), i32p]
        L.qadc_adc_search_exact_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
        L.qadc_refine_create_sq8.argtypes = [C.POINTER(C.c_void_p), C.c_int, f32p, f32p, C.c_int, C.c_int]
        L.qadc_refine_sq_range_host.argtypes = [f32p, C.c_uint64, C.c_int, C.c_int, f32p, f32p]
        L.qadc_refine_sq_range_device.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, f32p, f32p]
        L.qadc_refine_sq_info.argtypes = [C.c_void_p, f32p, f32p, u64p]
        L.qadc_refine_get.argtypes = [C.c_void_p, u32p, C.c_uint64, f32p, C.POINTER(C.c_uint8)]
        L.qadc_refine_get_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.qadc_pq_decode_host.argtypes = [C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_int, f32p, i32p, C.c_void_p, C.c_uint64, f32p, f32p, f32p,
                                          C.c_int]
        L.qadc_pq_decode_device.argtypes = [C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_int, f32p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_int]
        L.qadc_adc_index_reconstruct.argtypes = [C.c_void_p, u32p, C.c_uint64, f32p, u64p]
        L.qadc_adc_index_reconstruct_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.qadc_adc_index_reconstruct_rows.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, f32p]
        L.qadc_adc_index_reconstruct_rows_device.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]
        L.qadc_refine_range.argtypes = [C.c_void_p, C.c_int, f32p, f32p, C.c_void_p, u64p]
        L.qadc_refine_range_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, f32p, C.c_void_p, u64p]
        L.qadc_refine_rerank_range.argtypes = [C.c_void_p, C.c_int, f32p, u64p, u32p, f32p, u64p, u64p]
        L.qadc_refine_rerank_range_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, u64p, C.c_void_p, f32p, u64p, u64p]
        L.qadc_refine_range_collect.argtypes = [C.c_void_p, C.c_uint64, u32p, f32p]
        L.qadc_refine_range_collect_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.qadc_refine_set_range_plan.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int]
        L.qadc_refine_range_reruns.argtypes = [C.c_void_p]
        L.qadc_refine_range_reruns.restype = C.c_uint64
        _lib = L
    return _lib


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _check(rc):
    if rc != 0:
        raise QadcError("qadc error %d: %s" % (rc, lib().qadc_last_error().decode()))


def _add_labels(labels, n, labels_offset):
    """the labels of an add_vectors(labels=...) call: a uint32 array [n], given without a labels_offset"""
    if labels_offset != 0:
        raise ValueError("labels and a non-zero labels_offset exclude each other: labels[i] is the whole label of vector i")
    if not isinstance(labels, np.ndarray) or labels.dtype != np.uint32:
        raise ValueError("labels must be a numpy uint32 array, not %s" % (getattr(labels, "dtype", type(labels).__name__),))
    if labels.ndim != 1 or labels.shape[0] != n:
        raise ValueError("labels has shape %s, expected [%d]: one label per vector" % (tuple(labels.shape), n))
    return np.ascontiguousarray(labels)


def _add_labels_tensor(t, n, labels_offset, device):
    """the labels of an add_vectors_device(labels=...) call: a contiguous 1-d int32 torch tensor [n] on `device` that carries the
    labels' uint32 bits (the form in which search_device returns keys), or a uint32 one"""
    import torch
    if labels_offset != 0:
        raise ValueError("labels and a non-zero labels_offset exclude each other: labels[i] is the whole label of vector i")
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
        raise ValueError("labels must be an int32 torch.Tensor (the uint32 bits), not %s" % (getattr(t, "dtype", type(t).__name__),))
    if t.ndim != 1 or int(t.shape[0]) != n:
        raise ValueError("labels has shape %s, expected [%d]: one label per vector" % (tuple(t.shape), n))
    if t.device.type != "cuda" or t.device.index != device:
        raise QadcError("labels is on %s; the index is on device %d" % (t.device, device))
    if not t.is_contiguous():
        raise QadcError("labels must be contiguous")
    torch.cuda.current_stream(t.device).synchronize()                    # the labels are complete before the call
    return t


def _label_tensor(t, device):
    """the list of a remove_labels_device call: a contiguous 1-d int32 torch tensor on `device` carrying the labels' uint32 bits"""
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError("labels must be a torch.Tensor, not %s" % type(t).__name__)
    if t.dtype != torch.int32:
        raise TypeError("labels must be int32 (the uint32 bits, as search_device returns keys), not %s" % t.dtype)
    if t.device.type != "cuda" or t.device.index != device:
        raise QadcError("labels is on %s; the index is on device %d" % (t.device, device))
    if t.ndim != 1:
        raise QadcError("labels has shape %s, expected [n]" % (tuple(t.shape),))
    if not t.is_contiguous():
        raise QadcError("labels must be contiguous")
    torch.cuda.current_stream(t.device).synchronize()                    # the list is complete before the call
    return t


def replay_i8(keys, vals, R, sentinel=False):
    """Host-only heap replay (no GPU needed)."""
    keys = np.ascontiguousarray(keys, np.uint32)
    vals = np.ascontiguousarray(vals, np.int8)
    ok, ov, osz = np.zeros(R, np.uint32), np.zeros(R, np.int8), C.c_int32(0)
    _check(lib().qadc_replay_i8(len(keys), _p(keys, u32p), _p(vals, i8p), R, int(sentinel), _p(ok, u32p),
                                _p(ov, i8p), C.byref(osz)))
    return ok[:osz.value].copy(), ov[:osz.value].copy()


def device_prepare(device=0):
    """qadc_device_prepare: the library's per-device stream set, created now — call before any communicator is initialised."""
    _check(lib().qadc_device_prepare(int(device)))


def nib_choice(qtables, device=0):
    """qadc_nib_choice: the nibble form's choice bytes of 16x4 int8 tables [..., 16, 16] as the device computes them ->
    uint8 [ntables, 3, 4]: for NS = 8, 9, 10 the deferred mask (two bytes, low first), the slack, 0."""
    qt = np.ascontiguousarray(qtables, np.int8).reshape(-1, 256)
    out = np.zeros((qt.shape[0], 3, 4), np.uint8)
    _check(lib().qadc_nib_choice(int(device), qt.ctypes.data_as(C.c_void_p), int(qt.shape[0]), out.ctypes.data_as(C.c_void_p)))
    return out


def bktw_choice(qtables, device=0):
    """qadc_bktw_choice: the wide bucket form's choice bytes of 16x4 int8 tables [..., 16, 16] as the device computes them ->
    uint8 [ntables, 4, 4]: for NSP = 3, 4, 5, 6 the deferred mask among sub-quantizers 5-15 (two bytes, low first), the slack, 0."""
    qt = np.ascontiguousarray(qtables, np.int8).reshape(-1, 256)
    out = np.zeros((qt.shape[0], 4, 4), np.uint8)
    _check(lib().qadc_bktw_choice(int(device), qt.ctypes.data_as(C.c_void_p), int(qt.shape[0]), out.ctypes.data_as(C.c_void_p)))
    return out


def bkt_choice(qtables, device=0):
    """qadc_bkt_choice: the bucket form's choice bytes of 16x4 int8 tables [..., 16, 16] as the device computes them ->
    uint8 [ntables, 4, 4]: for NSP = 4, 5, 6, 7 the deferred mask among sub-quantizers 4-15 (two bytes, low first), the slack, 0."""
    qt = np.ascontiguousarray(qtables, np.int8).reshape(-1, 256)
    out = np.zeros((qt.shape[0], 4, 4), np.uint8)
    _check(lib().qadc_bkt_choice(int(device), qt.ctypes.data_as(C.c_void_p), int(qt.shape[0]), out.ctypes.data_as(C.c_void_p)))
    return out


def option_names():
    """The names qadc_set_option accepts (qadc_option_names)."""
    f = lib().qadc_option_names
    f.restype = C.c_char_p
    return f().decode().split(",")


def stream_layout(device=0):
    """qadc_stream_layout: '<stream creation order kept> | <ok or the obstructed pairs>'."""
    f = lib().qadc_stream_layout
    f.restype = C.c_char_p
    return f(int(device)).decode()


def stream_probe(a, b, device=0):
    """qadc_stream_probe: (microseconds a one-wave marker on stream b waited behind a CU-hungry launch on stream a, that launch's
    duration).  Streams: 0 scan, 1 copy, 2 ordering, 3 front, 4 alternative scan, 5 collectives, 6 merge."""
    w, sp = C.c_double(0), C.c_double(0)
    _check(lib().qadc_stream_probe(int(device), int(a), int(b), C.byref(w), C.byref(sp)))
    return w.value, sp.value


def sort_keys_i8(heap_keys, heap_vals):
    """Host-only: kv_binheap::sort_keys of a heap array (binheap.hpp:129-137)."""
    k = np.ascontiguousarray(heap_keys, np.uint32)
    v = np.ascontiguousarray(heap_vals, np.int8)
    out = np.zeros(len(k), np.uint32)
    _check(lib().qadc_sort_keys_i8(len(k), _p(k, u32p), _p(v, i8p), _p(out, u32p)))
    return out


def dist_unique_id():
    """128-byte RCCL unique id (rank 0 creates it, the other ranks receive it by any means)."""
    uid = np.zeros(128, np.uint8)
    _check(lib().qadc_dist_unique_id(_p(uid, u8p)))
    return uid


class ShmTransport:
    """The library's built-in host-staged all-gather over a POSIX shared-memory segment (qadc_shm_transport_*): the
    transport of ranks that share one GPU or have no RCCL.  name: "/something", unique per run."""

    def __init__(self, name, rank, world, slot_bytes=64 << 20, timeout_s=120.0):
        self.rank, self.world = rank, world
        self._ctx = C.c_void_p()
        rc = lib().qadc_shm_transport_open(name.encode(), rank, world, slot_bytes, timeout_s, C.byref(self._ctx))
        if rc != 0:
            raise QadcError("qadc error %d: %s" % (rc, lib().qadc_shm_transport_error().decode()))

    def allgather_host(self, arr):
        """Host buffers only (no GPU): every rank's `arr` -> [world][...]."""
        a = np.ascontiguousarray(arr)
        out = np.zeros((self.world,) + a.shape, a.dtype)
        rc = lib().qadc_shm_transport_allgather_host(self._ctx, a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), a.nbytes)
        if rc != 0:
            raise QadcError("qadc error %d: %s" % (rc, lib().qadc_shm_transport_error().decode()))
        return out

    def close(self):
        if self._ctx:
            lib().qadc_shm_transport_close(self._ctx)
            self._ctx = C.c_void_p()


def place_partitions(sizes, world):
    """Size-balanced owner rank of every partition (qadc_place_partitions)."""
    sz = np.ascontiguousarray(sizes, np.uint32)
    owner = np.zeros(len(sz), np.int32)
    _check(lib().qadc_place_partitions(len(sz), _p(sz, u32p), world, _p(owner, i32p)))
    return owner


def dist_merge_blocks(streams, nq, ma, R, device=0, host=False):
    """streams[g] = dict(keys, vals, slots, offsets) of virtual rank g (Index.query_scan_shard_streams): assembles the
    blocks qadc_dist_collect would gather and runs the device-side merge (host=True: the host-share replay the ranks
    run for few-query batches, all ranks' shares in turn).  -> list of (keys, values) heaps."""
    world = len(streams)
    cap = max(int(st["offsets"][-1]) for st in streams) + 3
    bw = 2 * nq + cap
    g = np.zeros((world, bw), np.uint64)
    for r, st in enumerate(streams):
        hdr = g[r, :2 * nq].view(np.uint32).reshape(nq, 4)
        off = st["offsets"].astype(np.int64)
        hdr[:, 0] = off[:-1]
        hdr[:, 1] = np.diff(off)
        hdr[:, 2] = 4
        tot = int(off[-1])
        ent = st["keys"][:tot].astype(np.uint64) | (st["vals"][:tot].astype(np.uint8).astype(np.uint64) << np.uint64(32)) | \
            (st["slots"][:tot].astype(np.uint64) << np.uint64(40))
        g[r, 2 * nq:2 * nq + tot] = ent
    keys = np.zeros((nq, R), np.uint32)
    vals = np.zeros((nq, R), np.int8)
    sizes = np.zeros(nq, np.int32)
    if host:
        _check(lib().qadc_dist_merge_blocks_host(world, nq, ma, R, _p(g, u64p), bw, _p(keys, u32p), _p(vals, i8p), _p(sizes, i32p)))
    else:
        _check(lib().qadc_dist_merge_blocks(device, world, nq, ma, R, _p(g, u64p), bw, _p(keys, u32p), _p(vals, i8p), _p(sizes, i32p)))
    return [(keys[q, :sizes[q]].copy(), vals[q, :sizes[q]].copy()) for q in range(nq)]


def merge_streams_i8(gathered, world, nq, R, cap, ma, q_first, q_step, status, keys, vals, sizes):
    """Host-only: replay the queries q_first, q_first+q_step, ... of the gathered per-rank streams (sharded.py)."""
    g = np.ascontiguousarray(gathered, np.int32).reshape(world, -1)
    st = None if status is None else np.ascontiguousarray(status, np.int32)
    _check(lib().qadc_merge_streams_i8(world, nq, R, cap, ma, _p(g, i32p), g.shape[1], q_first, q_step, _p(st, i32p),
                                       _p(keys, u32p), _p(vals, i8p), _p(sizes, i32p)))


def ivf_encode(codebooks, vectors, coarse=None, rotation=None, device=0, encode_form=1, sum_mode=1):
    """index_db::add_vectors' compute on the GPU: nearest coarse centroid, residual, optional OPQ rotation, PQ encode.
    -> (assign int32 [n] or None for a flat database, codes uint8 [n][M/2]).  encode_form / sum_mode: see pq_encode."""
    cb = np.ascontiguousarray(codebooks, np.float32)
    v = np.ascontiguousarray(vectors, np.float32)
    M, dim, n = cb.shape[0], v.shape[1], v.shape[0]
    co = None if coarse is None else np.ascontiguousarray(coarse, np.float32)
    rot = None if rotation is None else np.ascontiguousarray(rotation, np.float32)
    assert rot is None or rot.shape == (dim, dim)
    K = 0 if co is None else co.shape[0]
    assign = np.zeros(n, np.int32) if K else None
    codes = np.zeros((n, M // 2), np.uint8)
    _check(lib().qadc_ivf_encode_host_mode(M, dim, _p(cb, f32p), _p(rot, f32p), K, _p(co, f32p), _p(v, f32p), n, _p(assign, i32p),
                                           _p(codes, u8p), encode_form, sum_mode, device))
    return assign, codes


def kmeans_iterations(vectors, centroids, iters, device=0, div_mode=1):
    """kmeans_fast_iterations_thread on the GPU: -> (centroids float32 [K][dim], assign int32 [n] of the last round).
    div_mode 1: centroid = sum * (1 / count) as the reference is compiled (-ffast-math); 0: the source's division."""
    v = np.ascontiguousarray(vectors, np.float32)
    c = np.array(centroids, np.float32, order="C", copy=True)
    assign = np.zeros(v.shape[0], np.int32)
    _check(lib().qadc_kmeans_iterations_host_mode(_p(v, f32p), v.shape[0], v.shape[1], c.shape[0], _p(c, f32p), iters, _p(assign, i32p),
                                                  div_mode, device))
    return c, assign


def _train_pq_args(dim, codebooks_seed, bits, coarse, rotation):
    cb = np.array(codebooks_seed, np.float32, order="C", copy=True)
    if cb.ndim != 3:
        raise QadcError("codebooks_seed has shape %s, expected [sq_count][2^bits][dim / sq_count]" % (tuple(cb.shape),))
    if bits is None:
        bits = {16: 4, 256: 8, 65536: 16}.get(cb.shape[1])
        if bits is None:
            raise QadcError("cannot infer bits from %d centroids per sub-quantizer (16 or 256)" % cb.shape[1])
    if cb.shape[1] != 1 << bits or cb.shape[0] * cb.shape[2] != dim:
        raise QadcError("codebooks_seed has shape %s, expected [sq_count][%d][%d / sq_count]" % (tuple(cb.shape), 1 << bits, dim))
    co = None if coarse is None else np.ascontiguousarray(coarse, np.float32)
    rot = None if rotation is None else np.ascontiguousarray(rotation, np.float32)
    if rot is not None and rot.shape != (dim, dim):
        raise QadcError("rotation has shape %s, expected [%d][%d]" % (tuple(rot.shape), dim, dim))
    if co is not None and (co.ndim != 2 or co.shape[1] != dim):
        raise QadcError("coarse has shape %s, expected [K][%d]" % (tuple(co.shape), dim))
    return cb, bits, co, rot


def _repair_result(out, repair, repaired):
    return out + (int(repaired.value),) if repair else out


def train_pq(vectors, codebooks_seed, iters, bits=None, coarse=None, rotation=None, device=0, div_mode=1, sum_mode=1, repair=False):
    """Learn a product quantizer on the GPU (qadc_pq_train_host): `iters` rounds of kmeans_fast_iterations_thread in every sub-space
    at once, from the caller's seed [sq_count][2^bits][dim / sq_count] (pq_seed); bits (4 or 8) is inferred from the seed's second
    axis.  With coarse [K][dim] the learning set is first made residuals to the nearest coarse centroid, with rotation
    [dim][dim] those are rotated.  -> (codebooks float32 like the seed, codes uint8 of the last round in the encoder's layout —
    [n][sq_count / 2] packed nibbles at 4 bits, [n][sq_count] at 8 —, empty = centroids that are NaN at return).
    repair=True (qadc_pq_train_repair_host): every round refills its empty clusters between the assignment and the update
    (include/qadc.h "Empty-cluster repair"), and the tuple gains a last element `repaired`, the vectors moved in all rounds."""
    v = np.ascontiguousarray(vectors, np.float32)
    if v.ndim != 2:
        raise QadcError("vectors has shape %s, expected [n][dim]" % (tuple(v.shape),))
    n, dim = v.shape
    cb, bits, co, rot = _train_pq_args(dim, codebooks_seed, bits, coarse, rotation)
    nsq = cb.shape[0]
    codes = np.zeros((n, nsq // 2 if bits == 4 else nsq), np.uint8)
    empty, repaired = C.c_uint64(0), C.c_uint64(0)
    _check(lib().qadc_pq_train_repair_host(_p(v, f32p), n, dim, nsq, bits, 0 if co is None else co.shape[0], _p(co, f32p), _p(rot, f32p),
                                           _p(cb, f32p), iters, codes.ctypes.data_as(C.c_void_p), C.byref(empty), div_mode, sum_mode,
                                           int(bool(repair)), C.byref(repaired), device))
    return _repair_result((cb, codes, int(empty.value)), repair, repaired)


def train_pq_device(vectors, codebooks_seed, iters, bits=None, coarse=None, rotation=None, div_mode=1, sum_mode=1, repair=False):
    """train_pq on a learning set already in device memory: a contiguous float32 [n][dim] torch tensor on a GPU (read only).  The
    seed, coarse and rotation are host arrays; the results come back as numpy arrays like train_pq's."""
    import torch
    if not isinstance(vectors, torch.Tensor):
        raise TypeError("vectors must be a torch.Tensor, not %s" % type(vectors).__name__)
    if vectors.dtype != torch.float32:
        raise TypeError("vectors must be float32, not %s" % vectors.dtype)
    if vectors.device.type != "cuda":
        raise QadcError("vectors is on %s; train_pq_device takes a tensor in device memory" % vectors.device)
    if vectors.ndim != 2 or not vectors.is_contiguous():
        raise QadcError("vectors must be a contiguous [n][dim] tensor")
    n, dim = int(vectors.shape[0]), int(vectors.shape[1])
    cb, bits, co, rot = _train_pq_args(dim, codebooks_seed, bits, coarse, rotation)
    nsq = cb.shape[0]
    codes = np.zeros((n, nsq // 2 if bits == 4 else nsq), np.uint8)
    empty, repaired = C.c_uint64(0), C.c_uint64(0)
    torch.cuda.current_stream(vectors.device).synchronize()                # the learning set is complete before the call
    _check(lib().qadc_pq_train_repair_device(C.c_void_p(vectors.data_ptr()), n, dim, nsq, bits, 0 if co is None else co.shape[0], _p(co, f32p),
                                             _p(rot, f32p), _p(cb, f32p), iters, codes.ctypes.data_as(C.c_void_p), C.byref(empty), div_mode,
                                             sum_mode, int(bool(repair)), C.byref(repaired), vectors.device.index or 0))
    return _repair_result((cb, codes, int(empty.value)), repair, repaired)


def _train_pq16_args(dim, codebooks_seed, coarse, rotation):
    cb, bits, co, rot = _train_pq_args(dim, codebooks_seed, None, coarse, rotation)
    if bits != 16:
        raise QadcError("codebooks_seed has shape %s, expected [sq_count][65536][dim / sq_count] (train_pq learns 4- and 8-bit "
                        "sub-quantizers)" % (tuple(cb.shape),))
    return cb, co, rot


def train_pq16(vectors, codebooks_seed, iters, coarse=None, rotation=None, device=0, div_mode=1, sum_mode=1, repair=False):
    """Learn a product quantizer of 16-bit sub-quantizers on the GPU (qadc_pq_train16_host): train_pq with a seed
    [sq_count][65536][dim / sq_count], sq_count 2, 4 or 8 (pq_seed(v, sq_count, 16, rng)).  A round is the 16-bit encoder and the
    sorted centroid update.  -> (codebooks float32 like the seed, codes uint16 [n][sq_count] of the last round — adc_encode16's
    layout —, empty = centroids that are NaN at return).  repair=True (qadc_pq_train16_repair_host): as for train_pq, the tuple
    gains `repaired`."""
    v = np.ascontiguousarray(vectors, np.float32)
    if v.ndim != 2:
        raise QadcError("vectors has shape %s, expected [n][dim]" % (tuple(v.shape),))
    n, dim = v.shape
    cb, co, rot = _train_pq16_args(dim, codebooks_seed, coarse, rotation)
    nsq = cb.shape[0]
    codes = np.zeros((n, nsq), "<u2")
    empty, repaired = C.c_uint64(0), C.c_uint64(0)
    _check(lib().qadc_pq_train16_repair_host(_p(v, f32p), n, dim, nsq, 0 if co is None else co.shape[0], _p(co, f32p), _p(rot, f32p), _p(cb, f32p),
                                             iters, codes.ctypes.data_as(C.c_void_p), C.byref(empty), div_mode, sum_mode, int(bool(repair)),
                                             C.byref(repaired), device))
    return _repair_result((cb, codes.astype(np.uint16, copy=False), int(empty.value)), repair, repaired)


def train_pq16_device(vectors, codebooks_seed, iters, coarse=None, rotation=None, div_mode=1, sum_mode=1, repair=False):
    """train_pq16 on a learning set already in device memory: a contiguous float32 [n][dim] torch tensor on a GPU (read only).  The
    seed, coarse and rotation are host arrays; the results come back as numpy arrays like train_pq16's."""
    import torch
    if not isinstance(vectors, torch.Tensor):
        raise TypeError("vectors must be a torch.Tensor, not %s" % type(vectors).__name__)
    if vectors.dtype != torch.float32:
        raise TypeError("vectors must be float32, not %s" % vectors.dtype)
    if vectors.device.type != "cuda":
        raise QadcError("vectors is on %s; train_pq16_device takes a tensor in device memory" % vectors.device)
    if vectors.ndim != 2 or not vectors.is_contiguous():
        raise QadcError("vectors must be a contiguous [n][dim] tensor")
    n, dim = int(vectors.shape[0]), int(vectors.shape[1])
    cb, co, rot = _train_pq16_args(dim, codebooks_seed, coarse, rotation)
    nsq = cb.shape[0]
    codes = np.zeros((n, nsq), "<u2")
    empty, repaired = C.c_uint64(0), C.c_uint64(0)
    torch.cuda.current_stream(vectors.device).synchronize()                # the learning set is complete before the call
    _check(lib().qadc_pq_train16_repair_device(C.c_void_p(vectors.data_ptr()), n, dim, nsq, 0 if co is None else co.shape[0], _p(co, f32p),
                                               _p(rot, f32p), _p(cb, f32p), iters, codes.ctypes.data_as(C.c_void_p), C.byref(empty), div_mode,
                                               sum_mode, int(bool(repair)), C.byref(repaired), vectors.device.index or 0))
    return _repair_result((cb, codes.astype(np.uint16, copy=False), int(empty.value)), repair, repaired)


def pq_update16(vectors, codes, sq_count, div_mode=1, device=0):
    """The centroid update of train_pq16 alone (qadc_pq_update16_host), from codes the caller gives: vectors [n][dim] as the
    quantizer sees them, codes uint16 [n][sq_count] -> (codebooks float32 [sq_count][65536][dim / sq_count], NaN where a cluster
    is empty, counts uint32 [sq_count][65536])."""
    v = np.ascontiguousarray(vectors, np.float32)
    c = np.ascontiguousarray(codes, "<u2")
    if v.ndim != 2 or c.shape != (v.shape[0], sq_count):
        raise QadcError("vectors %s and codes %s: expected [n][dim] and [n][%d]" % (tuple(v.shape), tuple(c.shape), sq_count))
    n, dim = v.shape
    if sq_count <= 0 or dim % sq_count:
        raise QadcError("dim %d is not a multiple of sq_count %d" % (dim, sq_count))
    cb = np.zeros((sq_count, 65536, dim // sq_count), np.float32)
    counts = np.zeros((sq_count, 65536), np.uint32)
    _check(lib().qadc_pq_update16_host(_p(v, f32p), n, dim, sq_count, c.ctypes.data_as(C.c_void_p), _p(cb, f32p), _p(counts, u32p), div_mode,
                                       device))
    return cb, counts


def pq_repair(vectors, codebooks, codes, device=0):
    """The empty-cluster repair of the training rounds alone (qadc_pq_repair_host; include/qadc.h "Empty-cluster repair"): vectors
    [n][dim] as the quantizer sees them, codebooks [sq_count][2^bits][dim / sq_count] (bits 4, 8 or 16 from the second axis), codes in
    the encoder's layout (uint8 [n][sq_count / 2] packed nibbles, uint8 [n][sq_count], or uint16 [n][sq_count]) -> (codes with every
    empty cluster given the farthest eligible vector, moved uint32 [sq_count])."""
    v = np.ascontiguousarray(vectors, np.float32)
    if v.ndim != 2:
        raise QadcError("vectors has shape %s, expected [n][dim]" % (tuple(v.shape),))
    n, dim = v.shape
    cb, bits, _, _ = _train_pq_args(dim, codebooks, None, None, None)
    nsq = cb.shape[0]
    c = np.array(codes, "<u2" if bits == 16 else np.uint8, order="C", copy=True)
    if c.shape != (n, nsq // 2 if bits == 4 else nsq):
        raise QadcError("codes has shape %s, expected the encoder's layout [%d][%d]" % (tuple(c.shape), n, nsq // 2 if bits == 4 else nsq))
    moved = np.zeros(nsq, np.uint32)
    _check(lib().qadc_pq_repair_host(_p(v, f32p), n, dim, nsq, bits, _p(cb, f32p), c.ctypes.data_as(C.c_void_p), _p(moved, u32p), device))
    return (c.astype(np.uint16, copy=False) if bits == 16 else c), moved


QADC_DECODE_CHUNK = 262144         # include/qadc.h: rows decoded per pass
QADC_RECONSTRUCT_MISSING = 0xFFFFFFFFFFFFFFFF   # include/qadc.h: where[i] of a key no row holds
DECODE_NAN_BITS = 0x7FC00000       # every float of a missing row


def _pq_decode_args(codebooks, coarse, rotation):
    cb = np.ascontiguousarray(codebooks, np.float32)
    if cb.ndim != 3:
        raise QadcError("codebooks has shape %s, expected [sq_count][2^bits][dim / sq_count]" % (tuple(cb.shape),))
    bits = {16: 4, 256: 8, 65536: 16}.get(cb.shape[1])
    if bits is None:
        raise QadcError("cannot infer bits from %d centroids per sub-quantizer (16, 256 or 65536)" % cb.shape[1])
    dim = cb.shape[0] * cb.shape[2]
    co = None if coarse is None else np.ascontiguousarray(coarse, np.float32)
    rot = None if rotation is None else np.ascontiguousarray(rotation, np.float32)
    if rot is not None and rot.shape != (dim, dim):
        raise QadcError("rotation has shape %s, expected [%d][%d]" % (tuple(rot.shape), dim, dim))
    if co is not None and (co.ndim != 2 or co.shape[1] != dim):
        raise QadcError("coarse has shape %s, expected [K][%d]" % (tuple(co.shape), dim))
    return cb, bits, dim, co, rot


def pq_decode(codebooks, codes, assign=None, coarse=None, rotation=None, vectors=None, device=0):
    """PQ codes back to vectors on the GPU (qadc_pq_decode_host; include/qadc.h "Reconstruction"): the inverse of ivf_encode,
    adc_encode and adc_encode16.  codebooks [sq_count][2^bits][dim / sq_count] (bits 4, 8 or 16 from the second axis), codes in the
    encoder's layout (uint8 [n][sq_count / 2] packed nibbles, uint8 [n][sq_count], or uint16 [n][sq_count]), assign int32 [n] with
    coarse [K][dim] (a row whose entry lies outside [0, K) comes back as a missing row, every float 0x7FC00000), rotation [dim][dim].
    -> vectors float32 [n][dim]; with vectors= (the originals) -> (vectors, err float32 [n]), err[i] the squared distance between
    vectors[i] and its reconstruction as one fmaf chain."""
    cb, bits, dim, co, rot = _pq_decode_args(codebooks, coarse, rotation)
    nsq = cb.shape[0]
    c = np.ascontiguousarray(codes, "<u2" if bits == 16 else np.uint8)
    cols = nsq // 2 if bits == 4 else nsq
    if c.ndim != 2 or c.shape[1] != cols:
        raise QadcError("codes has shape %s, expected the encoder's layout [n][%d]" % (tuple(c.shape), cols))
    n = c.shape[0]
    a = None if assign is None else np.ascontiguousarray(assign, np.int32).reshape(-1)
    if a is not None and a.shape[0] != n:
        raise QadcError("assign has %d entries for %d codes" % (a.shape[0], n))
    v = None if vectors is None else np.ascontiguousarray(vectors, np.float32)
    if v is not None and v.shape != (n, dim):
        raise QadcError("vectors has shape %s, expected [%d][%d]" % (tuple(v.shape), n, dim))
    out = np.zeros((n, dim), np.float32)
    err = None if v is None else np.zeros(n, np.float32)
    _check(lib().qadc_pq_decode_host(nsq, bits, dim, _p(cb, f32p), _p(rot, f32p), 0 if co is None else co.shape[0], _p(co, f32p), _p(a, i32p),
                                     c.ctypes.data_as(C.c_void_p), n, _p(v, f32p), _p(out, f32p), _p(err, f32p), device))
    return out if v is None else (out, err)


def pq_decode_device(codebooks, codes, assign=None, coarse=None, rotation=None, vectors=None, out=None):
    """pq_decode from and to device memory (qadc_pq_decode_device): codes a contiguous uint8 torch tensor [n][code bytes] on a GPU
    (16-bit codes as their little-endian bytes, [n][2 * sq_count], or an int16 tensor [n][sq_count] carrying the uint16 bits), assign
    an int32 tensor [n], vectors a float32 tensor [n][dim], all on that GPU and read where they lie.  -> a float32 tensor [n][dim]
    (out=: written into it), with vectors= -> (that, err float32 tensor [n]).  The quantizers are host arrays."""
    import torch
    cb, bits, dim, co, rot = _pq_decode_args(codebooks, coarse, rotation)
    nsq = cb.shape[0]
    if not isinstance(codes, torch.Tensor) or codes.device.type != "cuda" or codes.ndim != 2 or not codes.is_contiguous():
        raise QadcError("codes must be a contiguous 2-d torch.Tensor in device memory")
    width = codes.shape[1] * codes.element_size()
    if codes.dtype not in (torch.uint8, torch.int16) or width != (nsq // 2 if bits == 4 else nsq if bits == 8 else 2 * nsq):
        raise QadcError("codes is %s %s, expected rows of %d code bytes" % (codes.dtype, tuple(codes.shape), nsq // 2 if bits == 4 else nsq * bits // 8))
    dev, n = codes.device, int(codes.shape[0])

    def there(t, dtype, shape, what):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != dev or not t.is_contiguous() or tuple(t.shape) != shape:
            raise QadcError("%s must be a contiguous %s tensor %s on %s" % (what, dtype, shape, dev))
        return t

    a = there(assign, torch.int32, (n,), "assign")
    v = there(vectors, torch.float32, (n, dim), "vectors")
    res = there(out, torch.float32, (n, dim), "out")
    if res is None:
        res = torch.zeros((n, dim), dtype=torch.float32, device=dev)
    err = None if v is None else torch.zeros((n,), dtype=torch.float32, device=dev)
    torch.cuda.current_stream(dev).synchronize()                         # the inputs and the zero fills are complete before the call
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    if n:                                                                # (an empty tensor has no address to pass)
        _check(lib().qadc_pq_decode_device(nsq, bits, dim, _p(cb, f32p), _p(rot, f32p), 0 if co is None else co.shape[0], _p(co, f32p), ptr(a),
                                           ptr(codes), n, ptr(v), ptr(res), ptr(err), dev.index or 0))
    return res if v is None else (res, err)


def quant_error(vectors, assign, codes, codebooks, coarse=None, rotation=None, device=0):
    """The distortion of a quantizer on vectors it encoded (the k-means objective the trainers minimise): vectors [n][dim], their
    coarse assignment (None without a coarse quantizer) and codes as the encoders and trainers return them
    -> (err float32 [n], total float64): err[i] = |vectors[i] - its reconstruction|^2 as pq_decode defines it, total the sum of
    err in float64 in ascending i (no total is formed on the device)."""
    _, err = pq_decode(codebooks, codes, assign=assign, coarse=coarse, rotation=rotation, vectors=vectors, device=device)
    total = 0.0
    for e in err.astype(np.float64):
        total += float(e)
    return err, np.float64(total)


QADC_OPQ_BLOCK = 2048              # include/qadc.h: vectors per float partial sum of the OPQ cross matrix


def _device_vectors(vectors, who):
    import torch
    if not isinstance(vectors, torch.Tensor):
        raise TypeError("vectors must be a torch.Tensor, not %s" % type(vectors).__name__)
    if vectors.dtype != torch.float32:
        raise TypeError("vectors must be float32, not %s" % vectors.dtype)
    if vectors.device.type != "cuda":
        raise QadcError("vectors is on %s; %s takes a tensor in device memory" % (vectors.device, who))
    if vectors.ndim != 2 or not vectors.is_contiguous():
        raise QadcError("vectors must be a contiguous [n][dim] tensor")
    torch.cuda.current_stream(vectors.device).synchronize()                # the learning set is complete before the call
    return int(vectors.shape[0]), int(vectors.shape[1])


def _opq_cross_args(n, dim, codes, codebooks, coarse):
    cb, bits, co, _ = _train_pq_args(dim, codebooks, None, coarse, None)
    nsq = cb.shape[0]
    c = np.ascontiguousarray(codes, np.uint8)
    if c.shape != (n, nsq // 2 if bits == 4 else nsq):
        raise QadcError("codes has shape %s, expected the encoder's layout [%d][%d]" % (tuple(c.shape), n, nsq // 2 if bits == 4 else nsq))
    return cb, bits, co, c


def opq_cross(vectors, codes, codebooks, coarse=None, device=0, sum_mode=1):
    """The cross matrix of OPQ learning on the GPU (qadc_opq_cross_host): M = X0^T Y, float64 [dim][dim], between the learning set
    as the quantizer sees it before rotation (X0: residuals to the nearest of coarse [K][dim] where given) and its reconstruction
    Y[i] = the centroids `codes` [n] (the encoder's layout, as train_pq returns them) select in codebooks
    [sq_count][2^bits][dim / sq_count].  Per block of QADC_OPQ_BLOCK vectors a float fmaf chain in vector order, the blocks added in
    float64."""
    v = np.ascontiguousarray(vectors, np.float32)
    if v.ndim != 2:
        raise QadcError("vectors has shape %s, expected [n][dim]" % (tuple(v.shape),))
    n, dim = v.shape
    cb, bits, co, c = _opq_cross_args(n, dim, codes, codebooks, coarse)
    M = np.zeros((dim, dim), np.float64)
    _check(lib().qadc_opq_cross_host(_p(v, f32p), n, dim, cb.shape[0], bits, 0 if co is None else co.shape[0], _p(co, f32p),
                                     c.ctypes.data_as(C.c_void_p), _p(cb, f32p), _p(M, C.POINTER(C.c_double)), sum_mode, device))
    return M


def opq_cross_device(vectors, codes, codebooks, coarse=None, sum_mode=1):
    """opq_cross on a learning set already in device memory: a contiguous float32 [n][dim] torch tensor on a GPU (read only).
    Everything else is a host array."""
    n, dim = _device_vectors(vectors, "opq_cross_device")
    cb, bits, co, c = _opq_cross_args(n, dim, codes, codebooks, coarse)
    M = np.zeros((dim, dim), np.float64)
    _check(lib().qadc_opq_cross_device(C.c_void_p(vectors.data_ptr()), n, dim, cb.shape[0], bits, 0 if co is None else co.shape[0],
                                       _p(co, f32p), c.ctypes.data_as(C.c_void_p), _p(cb, f32p), _p(M, C.POINTER(C.c_double)), sum_mode,
                                       vectors.device.index or 0))
    return M


def procrustes(M):
    """The orthogonal rotation that maximises tr(R M) (qadc_procrustes_host; host only): M float64 [dim][dim] ->
    (rotation float32 [dim][dim], Jacobi sweeps).  For M = opq_cross(...) it is the rotation under which the learning set is closest
    to its reconstruction."""
    m = np.ascontiguousarray(M, np.float64)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise QadcError("M has shape %s, expected [dim][dim]" % (tuple(m.shape),))
    rot = np.zeros(m.shape, np.float32)
    sweeps = C.c_int32(0)
    _check(lib().qadc_procrustes_host(_p(m, C.POINTER(C.c_double)), m.shape[0], _p(rot, f32p), C.byref(sweeps)))
    return rot, int(sweeps.value)


def _train_opq_args(n, dim, codebooks_seed, bits, coarse, rotation):
    cb, bits, co, rot = _train_pq_args(dim, codebooks_seed, bits, coarse, rotation)
    rot = np.eye(dim, dtype=np.float32) if rot is None else np.array(rot, np.float32, order="C", copy=True)
    nsq = cb.shape[0]
    return cb, bits, co, rot, np.zeros((n, nsq // 2 if bits == 4 else nsq), np.uint8)


def train_opq(vectors, codebooks_seed, outer, inner=1, rotation=None, coarse=None, bits=None, device=0, div_mode=1, sum_mode=1, repair=False):
    """Learn an OPQ rotation and its product quantizer on the GPU (qadc_opq_train_host): `outer` times [train_pq with `inner`
    rounds under the current rotation, opq_cross, procrustes], then `inner` closing rounds under the final rotation — bit for bit
    that loop of the public calls, with the learning set uploaded once.  rotation: the start [dim][dim] (None: the identity).
    -> (rotation float32 [dim][dim], codebooks, codes, empty, rounds_done) — codebooks, codes and empty as train_pq returns them;
    rounds_done < outer where a cross matrix was not finite (the rotation then stays as it was).  repair=True
    (qadc_opq_train_repair_host): the loop of train_pq(repair=True); the tuple gains a last element `repaired`."""
    v = np.ascontiguousarray(vectors, np.float32)
    if v.ndim != 2:
        raise QadcError("vectors has shape %s, expected [n][dim]" % (tuple(v.shape),))
    n, dim = v.shape
    cb, bits, co, rot, codes = _train_opq_args(n, dim, codebooks_seed, bits, coarse, rotation)
    empty, done, repaired = C.c_uint64(0), C.c_int32(0), C.c_uint64(0)
    _check(lib().qadc_opq_train_repair_host(_p(v, f32p), n, dim, cb.shape[0], bits, 0 if co is None else co.shape[0], _p(co, f32p), _p(rot, f32p),
                                            _p(cb, f32p), outer, inner, codes.ctypes.data_as(C.c_void_p), C.byref(empty), C.byref(done),
                                            div_mode, sum_mode, int(bool(repair)), C.byref(repaired), device))
    return _repair_result((rot, cb, codes, int(empty.value), int(done.value)), repair, repaired)


def train_opq_device(vectors, codebooks_seed, outer, inner=1, rotation=None, coarse=None, bits=None, div_mode=1, sum_mode=1, repair=False):
    """train_opq on a learning set already in device memory: a contiguous float32 [n][dim] torch tensor on a GPU (read only)."""
    n, dim = _device_vectors(vectors, "train_opq_device")
    cb, bits, co, rot, codes = _train_opq_args(n, dim, codebooks_seed, bits, coarse, rotation)
    empty, done, repaired = C.c_uint64(0), C.c_int32(0), C.c_uint64(0)
    _check(lib().qadc_opq_train_repair_device(C.c_void_p(vectors.data_ptr()), n, dim, cb.shape[0], bits, 0 if co is None else co.shape[0],
                                              _p(co, f32p), _p(rot, f32p), _p(cb, f32p), outer, inner, codes.ctypes.data_as(C.c_void_p),
                                              C.byref(empty), C.byref(done), div_mode, sum_mode, int(bool(repair)), C.byref(repaired),
                                              vectors.device.index or 0))
    return _repair_result((rot, cb, codes, int(empty.value), int(done.value)), repair, repaired)


def pq_seed(vectors, sq_count, bits, rng):
    """A seed for train_pq: the sub-vectors of 2^bits distinct rows of `vectors`, drawn with the numpy Generator `rng` ->
    float32 [sq_count][2^bits][dim / sq_count].  (Host only.)"""
    v = np.ascontiguousarray(vectors, np.float32)
    n, dim = v.shape
    K = 1 << bits
    if dim % sq_count or n < K:
        raise QadcError("pq_seed needs dim %% sq_count == 0 and at least %d vectors" % K)
    rows = v[rng.choice(n, K, replace=False)]
    return np.ascontiguousarray(rows.reshape(K, sq_count, dim // sq_count).transpose(1, 0, 2))


def _kmeans_seed_args(n, dim, k, sq_count, seed, coarse, rotation):
    if int(sq_count) != sq_count or sq_count < 1 or dim % sq_count:
        raise QadcError("dim %d is not a multiple of sq_count %s" % (dim, sq_count))
    if int(k) != k or k < 1 or k > n:
        raise QadcError("need 1 <= k <= n centres per sub-space, not k = %s with n = %d" % (k, n))
    if int(seed) != seed or not 0 <= seed < 2 ** 64:
        raise QadcError("seed must be an integer in [0, 2^64)")
    co = None if coarse is None else np.ascontiguousarray(coarse, np.float32)
    rot = None if rotation is None else np.ascontiguousarray(rotation, np.float32)
    if rot is not None and rot.shape != (dim, dim):
        raise QadcError("rotation has shape %s, expected [%d][%d]" % (tuple(rot.shape), dim, dim))
    if co is not None and (co.ndim != 2 or co.shape[1] != dim or co.shape[0] == 0):
        raise QadcError("coarse has shape %s, expected [K][%d]" % (tuple(co.shape), dim))
    sq_count, k = int(sq_count), int(k)
    return co, rot, np.zeros((sq_count, k, dim // sq_count), np.float32), np.zeros((sq_count, k), np.uint32)


def _kmeans_seed_result(centres, rows, fallbacks, return_rows):
    c = centres[0] if centres.shape[0] == 1 else centres
    return (c, rows[0] if centres.shape[0] == 1 else rows, int(fallbacks.value)) if return_rows else c


def kmeans_seed(vectors, k, sq_count=1, seed=0, coarse=None, rotation=None, device=0, return_rows=False):
    """k-means++ seeding on the GPU (qadc_kmeans_seed_host): k D^2 picks in each of sq_count sub-spaces at once, from the 64-bit
    `seed` (include/qadc.h states every bit).  With coarse [K][dim] the learning set is first made residuals to the nearest coarse
    centroid, with rotation [dim][dim] those are rotated, as the trainers do.  -> centres float32 [k][dim] for sq_count == 1 (a seed
    for kmeans_iterations), else [sq_count][k][dim / sq_count] (a seed for train_pq / train_pq16 / train_opq): the picked rows'
    sub-vectors, bit for bit.  return_rows: -> (centres, rows uint32 [k] or [sq_count][k], fallbacks) — fallbacks counts picks taken in
    index order because no weight was left (fewer distinct finite sub-vectors than k)."""
    v = np.ascontiguousarray(vectors, np.float32)
    if v.ndim != 2:
        raise QadcError("vectors has shape %s, expected [n][dim]" % (tuple(v.shape),))
    n, dim = v.shape
    co, rot, centres, rows = _kmeans_seed_args(n, dim, k, sq_count, seed, coarse, rotation)
    fallbacks = C.c_uint64(0)
    _check(lib().qadc_kmeans_seed_host(_p(v, f32p), n, dim, int(sq_count), int(k), 0 if co is None else co.shape[0], _p(co, f32p),
                                       _p(rot, f32p), int(seed), _p(centres, f32p), _p(rows, u32p), C.byref(fallbacks), device))
    return _kmeans_seed_result(centres, rows, fallbacks, return_rows)


def kmeans_seed_device(vectors, k, sq_count=1, seed=0, coarse=None, rotation=None, return_rows=False):
    """kmeans_seed on a learning set already in device memory: a contiguous float32 [n][dim] torch tensor on a GPU (read only).
    coarse and rotation are host arrays; the results come back as numpy arrays like kmeans_seed's."""
    n, dim = _device_vectors(vectors, "kmeans_seed_device")
    co, rot, centres, rows = _kmeans_seed_args(n, dim, k, sq_count, seed, coarse, rotation)
    fallbacks = C.c_uint64(0)
    _check(lib().qadc_kmeans_seed_device(C.c_void_p(vectors.data_ptr()), n, dim, int(sq_count), int(k), 0 if co is None else co.shape[0],
                                         _p(co, f32p), _p(rot, f32p), int(seed), _p(centres, f32p), _p(rows, u32p), C.byref(fallbacks),
                                         vectors.device.index or 0))
    return _kmeans_seed_result(centres, rows, fallbacks, return_rows)


def pq_seed_pp(vectors, sq_count, bits, seed, **kw):
    """A k-means++ seed for train_pq / train_pq16 / train_opq: kmeans_seed with k = 2^bits -> float32 [sq_count][2^bits][dim / sq_count]
    (pq_seed's shape; `seed` is an integer, and the keywords are kmeans_seed's)."""
    out = kmeans_seed(vectors, 1 << bits, sq_count=sq_count, seed=seed, **kw)
    if sq_count != 1:
        return out
    return (out[0][None], out[1][None], out[2]) if kw.get("return_rows") else out[None]


def coarse_assign(queries, coarse, ma, device=0):
    """find_k_neighbors with k = ma on the GPU, as qadc_search's front selects coarse centroids: queries [nq][dim], coarse
    [K][dim] -> assign int32 [nq][ma] (the reference's heap order, nearest first)."""
    q = np.ascontiguousarray(queries, np.float32)
    c = np.ascontiguousarray(coarse, np.float32)
    assert q.ndim == 2 and c.ndim == 2 and q.shape[1] == c.shape[1]
    assign = np.zeros((q.shape[0], ma), np.int32)
    _check(lib().qadc_coarse_assign_host(_p(q, f32p), q.shape[0], _p(c, f32p), c.shape[0], c.shape[1], ma, _p(assign, i32p), device))
    return assign


def pq_encode(codebooks, vectors, device=0, encode_form=1, sum_mode=1):
    """PQ-encode host vectors [n][dim] on the GPU -> uint8 codes [n][M/2].  encode_form 1 (default) = the reference's form
    (find_k_neighbors with k = 1 on the BLAS-expansion distances), 0 = direct sum (x - c)^2; sum_mode 1 = norms as compiled."""
    cb = np.ascontiguousarray(codebooks, np.float32)
    v = np.ascontiguousarray(vectors, np.float32)
    M, dim = cb.shape[0], v.shape[1]
    codes = np.zeros((v.shape[0], M // 2), np.uint8)
    _check(lib().qadc_pq_encode_host_mode(M, dim, _p(cb, f32p), _p(v, f32p), v.shape[0], _p(codes, u8p), encode_form, sum_mode, device))
    return codes


def adc_encode(codebooks, vectors, coarse=None, rotation=None, device=0, sum_mode=1):
    """Database build for 8-bit sub-quantizers on the GPU (qadc_adc_encode_host): nearest coarse centroid and residual (with
    coarse [K][dim]), OPQ rotation (with rotation [dim][dim]), one code byte per sub-quantizer.  codebooks [sq_count][256][dsq],
    vectors [n][dim] -> (assign int32 [n] or None for a flat database, codes uint8 [n][sq_count])."""
    cb = np.ascontiguousarray(codebooks, np.float32)
    v = np.ascontiguousarray(vectors, np.float32)
    assert cb.ndim == 3 and cb.shape[1] == 256 and v.ndim == 2
    nsq, dim, n = cb.shape[0], v.shape[1], v.shape[0]
    assert cb.shape[2] * nsq == dim
    co = None if coarse is None else np.ascontiguousarray(coarse, np.float32)
    rot = None if rotation is None else np.ascontiguousarray(rotation, np.float32)
    assert rot is None or rot.shape == (dim, dim)
    assert co is None or co.shape[1] == dim
    K = 0 if co is None else co.shape[0]
    assign = np.zeros(n, np.int32) if K else None
    codes = np.zeros((n, nsq), np.uint8)
    _check(lib().qadc_adc_encode_host(nsq, dim, _p(cb, f32p), _p(rot, f32p), K, _p(co, f32p), _p(v, f32p), n, sum_mode, _p(assign, i32p),
                                      _p(codes, u8p), device))
    return assign, codes


def adc_encode16(codebooks, vectors, coarse=None, rotation=None, device=0, sum_mode=1):
    """Database build for 16-bit sub-quantizers on the GPU (qadc_adc_encode16_host): adc_encode with codebooks
    [sq_count][65536][dsq], sq_count 2, 4 or 8.  vectors [n][dim] -> (assign int32 [n] or None for a flat database, codes uint16
    [n][sq_count]: viewed as uint8 [n][2 * sq_count] they are the rows add_partitions takes on an AdcIndex of 16-bit codes)."""
    cb = np.ascontiguousarray(codebooks, np.float32)
    v = np.ascontiguousarray(vectors, np.float32)
    assert cb.ndim == 3 and cb.shape[1] == 65536 and v.ndim == 2
    nsq, dim, n = cb.shape[0], v.shape[1], v.shape[0]
    assert cb.shape[2] * nsq == dim
    co = None if coarse is None else np.ascontiguousarray(coarse, np.float32)
    rot = None if rotation is None else np.ascontiguousarray(rotation, np.float32)
    assert rot is None or rot.shape == (dim, dim)
    assert co is None or co.shape[1] == dim
    K = 0 if co is None else co.shape[0]
    assign = np.zeros(n, np.int32) if K else None
    codes = np.zeros((n, nsq), "<u2")
    _check(lib().qadc_adc_encode16_host(nsq, dim, _p(cb, f32p), _p(rot, f32p), K, _p(co, f32p), _p(v, f32p), n, sum_mode,
                                        _p(assign, i32p), codes.ctypes.data_as(u8p), device))
    return assign, codes.astype(np.uint16, copy=False)


def pq_encode_device(codebooks, d_vectors_ptr, n, dim, d_codes_ptr, device=0):
    cb = np.ascontiguousarray(codebooks, np.float32)
    _check(lib().qadc_pq_encode(cb.shape[0], dim, _p(cb, f32p), C.c_void_p(d_vectors_ptr), n, C.c_void_p(d_codes_ptr), device))


class _RowStoreMixin:
    """db_add and remove by label, the same calls on both engines (DESIGN.md sections 11.5 to 11.7): Index binds them to qadc_index_*,
    AdcIndex to qadc_adc_index_*.  The class gives _c_prefix, _row_format() -> (values per row, dtype) of read_partition's codes, and
    _device_vectors(t) -> the checked torch tensor of add_vectors_device."""

    def _c(self, name):
        return getattr(lib(), self._c_prefix + name)

    # ---- db_add: encode and append on the GPU with the index's own quantizers (*_add_vectors) ----
    def add_vectors(self, vectors, labels_offset=0, sum_mode=1, labels=None):
        """vectors [n][dim]: with a coarse quantizer the code of vector i is appended to its nearest centroid's partition with label
        labels_offset + i (index_db::add_vectors); a flat index writes it at row labels_offset + i of its one partition
        (flat_db::add_vectors).  labels (a uint32 array [n], any values, repeats allowed; not together with a labels_offset): the
        label of vector i is labels[i] (*_add_vectors_labelled; an index with a coarse quantizer only).  A 4-bit Index is not
        finalized afterwards: call finalize before the next query."""
        v = np.ascontiguousarray(vectors, np.float32)
        if v.ndim == 1:
            v = v.reshape(-1, getattr(self, "dim", 1))
        assert v.ndim == 2 and (v.shape[0] == 0 or v.shape[1] == getattr(self, "dim", v.shape[1]))
        if labels is None:
            self.add_vectors_raw(v, v.shape[0], labels_offset, sum_mode)
        else:
            lab = _add_labels(labels, v.shape[0], labels_offset)
            _check(self._c("add_vectors_labelled")(self._h, _p(v, f32p), _p(lab, u32p), v.shape[0], sum_mode))

    def add_vectors_raw(self, vectors, count, labels_offset, sum_mode):
        """The C call as it is (vectors: a float32 array or None)."""
        _check(self._c("add_vectors")(self._h, _p(vectors, f32p), count, labels_offset, sum_mode))

    def add_vectors_device(self, vectors, labels_offset=0, sum_mode=1, labels=None):
        """add_vectors for a contiguous float32 torch tensor [n][dim] on the index's device, read where it lies; labels: an int32
        torch tensor [n] there that carries the labels' uint32 bits."""
        import torch
        v = self._device_vectors(vectors)
        n = int(v.shape[0])
        torch.cuda.current_stream(v.device).synchronize()                # the vectors are complete before the call
        if labels is None:
            _check(self._c("add_vectors_device")(self._h, v.data_ptr(), n, labels_offset, sum_mode))
        else:
            lab = _add_labels_tensor(labels, n, labels_offset, self.device)
            _check(self._c("add_vectors_labelled_device")(self._h, v.data_ptr(), lab.data_ptr(), n, sum_mode))

    def read_partition(self, part, first=0, count=None):
        """-> (codes, labels uint32 [n] or None on an index without labels): rows [first, first + count) of the partition as they
        lie in device memory (default: all of it).  codes: uint8 [n][M/2] of an Index, uint8 [n][sq_count] of an AdcIndex — a
        create16 index: uint16 [n][sq_count]."""
        if count is None:
            count = max(self.partition_size(part) - first, 0) if 0 <= part < self.partition_count() else 0
        width, dtype = self._row_format()
        codes = np.zeros((count, width), dtype)
        labels = np.zeros(count, np.uint32) if self._labelled() else None
        _check(self._c("read_partition")(self._h, part, first, count, _p(codes, u8p), _p(labels, u32p)))
        return (codes.astype(np.uint16, copy=False) if codes.dtype.itemsize == 2 else codes), labels

    def _labelled(self):
        """whether the database has labels: the C call fills labels_out only then (probed on the first row the index holds)"""
        for part in range(self.partition_count()):
            if self.partition_size(part):
                seen = []
                for fill in (0, 1):
                    one = np.full(1, fill, np.uint32)
                    _check(self._c("read_partition")(self._h, part, 0, 1, None, _p(one, u32p)))
                    seen.append(int(one[0]))
                return seen[0] == seen[1]
        return False

    def reserve(self, capacities):
        """minimum capacities, in codes, of the first len(capacities) partitions (empty ones are created where the index has fewer)"""
        c = np.ascontiguousarray(capacities, np.uint32).reshape(-1)
        _check(self._c("reserve")(self._h, len(c), _p(c, u32p)))

    def relocations(self):
        """add_vectors calls that had to move the database to grow it"""
        return self._c("relocations")(self._h)

    # ---- remove by label: the partitions compacted in place on the GPU (*_remove_labels) ----
    def remove_labels(self, labels):
        """Removes every row whose label is in `labels` (anything np.asarray(..., np.uint32) accepts) from whichever partitions
        hold it; the survivors keep their order.  -> the number of rows removed.  A call that removed a row leaves a 4-bit Index
        not finalized: call finalize before the next query."""
        l = np.ascontiguousarray(np.asarray(labels, np.uint32).reshape(-1))
        return self.remove_labels_raw(l, l.size)

    def remove_labels_raw(self, labels, count):
        """The C call as it is (labels: a uint32 array or None)."""
        removed = C.c_uint64(0)
        _check(self._c("remove_labels")(self._h, _p(labels, u32p), count, C.byref(removed)))
        return int(removed.value)

    def remove_labels_device(self, labels):
        """remove_labels for a contiguous 1-d int32 torch tensor on the index's device that carries the labels' uint32 bits — the
        form in which search_device returns keys — read where it lies."""
        t = _label_tensor(labels, self.device)
        removed = C.c_uint64(0)
        _check(self._c("remove_labels_device")(self._h, t.data_ptr(), int(t.shape[0]), C.byref(removed)))
        return int(removed.value)


class Index(_RowStoreMixin):
    """One GPU-resident Quick-ADC database (the role of scanner_4 after prepare_database)."""

    def __init__(self, M, device=0):
        self.M = M
        self.cs = M // 2
        self.device = device
        self._h = C.c_void_p()
        _check(lib().qadc_index_create(C.byref(self._h), M, device))
        self._keepalive = []

    def close(self):
        """Raises QadcError, and leaves the index open, while an AdcIndex.view_of(self) is still open."""
        if self._h:
            _check(lib().qadc_index_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- database --------------------------------------------------------------------------
    def add_partitions(self, codes, labels=None):
        codes = [np.ascontiguousarray(c, np.uint8).reshape(-1, self.cs) for c in codes]
        sizes = np.array([c.shape[0] for c in codes], np.uint32)
        ca = (u8p * len(codes))(*[_p(c, u8p) for c in codes])
        la = None
        if labels is not None:
            labels = [None if l is None else np.ascontiguousarray(l, np.uint32) for l in labels]
            la = (u32p * len(labels))(*[None if l is None else _p(l, u32p) for l in labels])
        _check(lib().qadc_index_add_partitions(self._h, len(codes), ca, la, _p(sizes, u32p)))

    def add_partition_interleaved(self, inter, size, labels=None):
        inter = np.ascontiguousarray(inter, np.uint8)
        lab = None if labels is None else np.ascontiguousarray(labels, np.uint32)
        _check(lib().qadc_index_add_partition_interleaved(self._h, _p(inter, u8p), _p(lab, u32p), size))

    def add_partition_device(self, d_codes_ptr, size, d_labels_ptr=None, keepalive=None):
        self._keepalive.append(keepalive)
        _check(lib().qadc_index_add_partition_device(self._h, C.c_void_p(d_codes_ptr),
                                                     C.c_void_p(d_labels_ptr) if d_labels_ptr else None, size))

    def add_partition_synthetic(self, size, seed, first_word=0):
        _check(lib().qadc_index_add_partition_synthetic(self._h, size, seed, first_word))

    def add_partition_shard(self, codes, local_first, global_n, labels=None, starts=None):
        codes = np.ascontiguousarray(codes, np.uint8).reshape(-1, self.cs)
        lab = None if labels is None else np.ascontiguousarray(labels, np.uint32)
        st = None if starts is None else np.ascontiguousarray(starts, np.uint8).reshape(-1, self.cs)
        _check(lib().qadc_index_add_partition_shard(self._h, _p(codes, u8p), _p(lab, u32p), codes.shape[0], global_n,
                                                    local_first, _p(st, u8p), 0 if st is None else st.shape[0]))

    def add_partition_synthetic_shard(self, global_n, first_pos, local_n, seed, starts_count):
        _check(lib().qadc_index_add_partition_synthetic_shard(self._h, global_n, first_pos, local_n, seed,
                                                              starts_count))

    def set_key_base(self, part, base):
        _check(lib().qadc_index_set_key_base(self._h, part, base))

    def finalize(self, keep):
        _check(lib().qadc_index_finalize(self._h, keep))

    def set_option(self, name, value):
        _check(lib().qadc_set_option(self._h, name.encode(), float(value)))

    def set_split(self, min_codes, min_run):
        """Split-scan thresholds (16x4): byte-plane copies for partitions of >= min_codes codes (0 = none; set before
        finalize), read by one-query-per-pass launches for runs of >= min_run codes."""
        _check(lib().qadc_index_set_split(self._h, int(min_codes), int(min_run)))

    def set_split6(self, min_run6):
        """Split launches whose runs all have >= min_run6 codes stream 6 of the 7 planes (0 = never); results do not change."""
        _check(lib().qadc_index_set_split6(self._h, int(min_run6)))

    def set_split5(self, min_run5):
        """Split launches whose runs all have >= min_run5 codes stream 5 of the 7 planes, preferred to the 6-plane form
        (0 = never); results do not change."""
        _check(lib().qadc_index_set_split5(self._h, int(min_run5)))

    def set_split_nib(self, min_run, min_run8=0, ns=9):
        """Nibble form (16x4): split launches whose runs all have >= min_run codes stream ns = 9 or 10 of the 16 sub-quantizers
        from a nibble-plane copy, those with >= min_run8 codes 8 of them; preferred to the 5-plane form (0 = never); results
        do not change.  Set before finalize: the copy (8 bytes per code) is built there."""
        _check(lib().qadc_index_set_split_nib(self._h, int(min_run), int(min_run8), int(ns)))

    def set_split_bkt(self, bkt_min_run, bkt_block=0, min_run6=0, min_run5=0, min_run4=0, bkt_max_pad=0.0):
        """Bucket form (16x4): finalize builds a bucket copy (blocks of bkt_block codes grouped by their first two bytes; about
        18.4 bytes per code) of partitions with >= bkt_min_run codes (0 = off); split launches whose runs all have >= bkt_min_run
        codes and cover whole blocks stream 7 of sub-quantizers 4-15, those with >= min_run6 / min_run5 / min_run4 codes 6 / 5 / 4
        (0 = never); preferred to the nibble form; results do not change.  bkt_block, bkt_max_pad: 0 = keep.  Turn the form on
        or off and set bkt_block before finalize."""
        _check(lib().qadc_index_set_split_bkt(self._h, int(bkt_min_run), int(bkt_block), int(min_run6), int(min_run5),
                                              int(min_run4), float(bkt_max_pad)))

    def set_split_bkt_wide(self, wide_block, min_run=0, min_run5=0, min_run4=0, min_run3=0, wide_max_pad=0.0):
        """Wide blocks of the bucket copy (16x4): finalize stores positions from wide_block = W on (0 = none; a power of two, a
        multiple of bkt_block) in octave blocks [W 2^j, W 2^(j+1)) grouped by the codes' first 20 bits, unless padding inflates an
        octave beyond wide_max_pad x its codes (0 = keep); split launches whose runs all have >= min_run codes and cover whole wide
        octaves stream 6 of sub-quantizers 5-15, those with >= min_run5 / min_run4 / min_run3 codes 5 / 4 / 3 (0 = never);
        preferred to the narrow form; results do not change.  Set wide_block and wide_max_pad before finalize."""
        _check(lib().qadc_index_set_split_bkt_wide(self._h, int(wide_block), int(min_run), int(min_run5), int(min_run4),
                                                   int(min_run3), float(wide_max_pad)))

    def set_bkt_prune(self, mode):
        """Group test of the wide form: 1 = wave iterations whose lane groups' free rows all reach the bound load no plane and look
        nothing up, 0 = the form without the test; results do not change."""
        _check(lib().qadc_index_set_bkt_prune(self._h, int(mode)))

    def set_bkt_prune_lanes(self, lanes):
        """Granularity of the group test's loads (with set_bkt_prune(1)): 16 = a 16-lane quarter of a running wave iteration none of
        whose lane groups keeps loads no plane either, 64 = whole wave iterations only; results do not change."""
        _check(lib().qadc_index_set_bkt_prune_lanes(self._h, int(lanes)))

    def set_bkt_tiles(self, mode):
        """Tile order of the bucket launches: 1 = strided tiles whatever bit 3 of "variant" says, 0 = they follow variant; results
        do not change."""
        _check(lib().qadc_index_set_bkt_tiles(self._h, int(mode)))

    def bktw_copy(self, part):
        """Diagnostic: partition part's wide octaves, or None.  -> dict(block = W, off uint64 [octaves + 1], tiles uint8
        [ntiles, 93184], codes uint8 [slots, 8], perm uint32 [slots]) (include/qadc.h: qadc_index_bktw_read)."""
        block, noct, slots = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().qadc_index_bktw_info(self._h, part, C.byref(block), C.byref(noct), C.byref(slots)))
        if not block.value:
            return None
        nt = slots.value // 16384
        off = np.zeros(noct.value + 1, np.uint64)
        tiles = np.zeros((nt, 93184), np.uint8)
        side = np.zeros((nt, 196608), np.uint8)
        _check(lib().qadc_index_bktw_read(self._h, part, _p(off, u64p), _p(tiles, u8p), _p(side, u8p)))
        codes = np.ascontiguousarray(side[:, :131072]).reshape(-1, 8)
        perm = np.ascontiguousarray(side[:, 131072:]).view(np.uint32).reshape(-1)
        return {"block": block.value, "off": off, "tiles": tiles, "codes": codes, "perm": perm}

    def bkt_copy(self, part):
        """Diagnostic: partition part's bucket copy, or None.  -> dict(block, off uint64 [blocks + 1], tiles uint8
        [ntiles, 100352], codes uint8 [slots, 8], perm uint32 [slots]) (include/qadc.h: qadc_index_bkt_read)."""
        block, nblocks, slots = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().qadc_index_bkt_info(self._h, part, C.byref(block), C.byref(nblocks), C.byref(slots)))
        if not block.value:
            return None
        nt = slots.value // 16384
        off = np.zeros(nblocks.value + 1, np.uint64)
        tiles = np.zeros((nt, 100352), np.uint8)
        side = np.zeros((nt, 196608), np.uint8)
        _check(lib().qadc_index_bkt_read(self._h, part, _p(off, u64p), _p(tiles, u8p), _p(side, u8p)))
        codes = np.ascontiguousarray(side[:, :131072]).reshape(-1, 8)
        perm = np.ascontiguousarray(side[:, 131072:]).view(np.uint32).reshape(-1)
        return {"block": block.value, "off": off, "tiles": tiles, "codes": codes, "perm": perm}

    def partition_count(self):
        return lib().qadc_index_partition_count(self._h)

    def partition_size(self, p):
        return lib().qadc_index_partition_size(self._h, p)

    def start_size(self, p):
        return lib().qadc_index_start_size(self._h, p)

    def read_codes(self, part, first, count):
        out = np.zeros((count, self.cs), np.uint8)
        _check(lib().qadc_index_read_codes(self._h, part, first, count, _p(out, u8p)))
        return out

    # ---- db_add and remove by label (qadc_index_add_vectors*, _reserve, _read_partition, _remove_labels*): _RowStoreMixin ----
    _c_prefix = "qadc_index_"

    def _row_format(self):
        return self.cs, np.uint8

    def _device_vectors(self, vectors):
        import torch
        if not isinstance(vectors, torch.Tensor) or vectors.ndim != 2:
            raise TypeError("vectors must be a 2-d torch.Tensor")
        if vectors.dtype != torch.float32:
            raise TypeError("vectors must be float32, not %s" % vectors.dtype)
        if vectors.device.type != "cuda" or vectors.device.index != self.device:
            raise QadcError("vectors is on %s; the index is on device %d" % (vectors.device, self.device))
        if not vectors.is_contiguous():
            raise QadcError("vectors must be contiguous")
        if vectors.shape[0] and int(vectors.shape[1]) != getattr(self, "dim", int(vectors.shape[1])):
            raise QadcError("vectors has shape %s, expected [n][%d]" % (tuple(vectors.shape), self.dim))
        return vectors

    # ---- queries ---------------------------------------------------------------------------
    @staticmethod
    def _prep(assign, nq=None):
        assign = np.ascontiguousarray(assign, np.int32)
        if assign.ndim == 1:
            assign = assign.reshape(1, -1) if nq is None else assign.reshape(nq, -1)
        return assign

    def _heaps(self, nq, R, keys, vals, sizes):
        return [(keys[q, :sizes[q]].copy(), vals[q, :sizes[q]].copy()) for q in range(nq)]

    def query_scan(self, assign, tables, R, want_qtables=False):
        """tables: float32 [nq][ma][M*16], mutated in place.  Returns dict with heaps etc."""
        assign = self._prep(assign)
        nq, ma = assign.shape
        assert tables.dtype == np.float32 and tables.flags.c_contiguous and tables.size == nq * ma * self.M * 16
        keys = np.zeros((nq, R), np.uint32)
        vals = np.zeros((nq, R), np.int8)
        sizes = np.zeros(nq, np.int32)
        status = np.zeros(nq, np.int32)
        qmin = np.zeros(nq, np.float32)
        qmax = np.zeros(nq, np.float32)
        qt = np.zeros((nq, ma, self.M, 16), np.int8) if want_qtables else None
        _check(lib().qadc_query_scan(self._h, nq, ma, _p(assign, i32p), _p(tables, f32p), R, _p(keys, u32p),
                                     _p(vals, i8p), _p(sizes, i32p), _p(status, i32p), _p(qmin, f32p),
                                     _p(qmax, f32p), _p(qt, i8p)))
        return dict(heaps=self._heaps(nq, R, keys, vals, sizes), status=status, qmin=qmin, qmax=qmax, qtables=qt,
                    keys=keys, values=vals, sizes=sizes)

    def submit(self, slot, assign, tables, R, prescan=None):
        """prescan: float32 [nq][w*R], the gathered output of prescan_collect on all w ranks (sharded pre-scan)."""
        assign = self._prep(assign)
        nq, ma = assign.shape
        assert tables.dtype == np.float32 and tables.flags.c_contiguous
        self._pending = getattr(self, "_pending", {})
        self._pending[slot] = (nq, R, tables, assign)
        if prescan is None:
            _check(lib().qadc_query_scan_submit(self._h, slot, nq, ma, _p(assign, i32p), _p(tables, f32p), R))
        else:
            pv = np.ascontiguousarray(prescan, np.float32).reshape(nq, -1)
            _check(lib().qadc_query_scan_submit_prescanned(self._h, slot, nq, ma, _p(assign, i32p), _p(tables, f32p), R,
                                                           _p(pv, f32p), pv.shape[1]))

    def prescan_submit(self, slot, assign, tables, R, slice_index, nslices):
        """Sharded pre-scan, first half: this rank's slice of the starts (own buffers: may overlap a pending batch)."""
        assign = self._prep(assign)
        nq, ma = assign.shape
        assert tables.dtype == np.float32 and tables.flags.c_contiguous
        self._pre_pending = getattr(self, "_pre_pending", {})
        self._pre_pending[slot] = (nq, R, tables, assign)
        _check(lib().qadc_prescan_submit(self._h, slot, nq, ma, _p(assign, i32p), _p(tables, f32p), R, slice_index, nslices))

    def prescan_collect(self, slot):
        """-> float32 [nq][R]: the R smallest pre-scan distances of the slice per query (FLT_MAX-padded)."""
        nq, R, tables, assign = self._pre_pending.pop(slot)
        vals = np.zeros((nq, R), np.float32)
        _check(lib().qadc_prescan_collect(self._h, slot, _p(vals, f32p)))
        return vals

    def collect(self, slot):
        nq, R, tables, assign = self._pending.pop(slot)
        keys = np.zeros((nq, R), np.uint32)
        vals = np.zeros((nq, R), np.int8)
        sizes = np.zeros(nq, np.int32)
        status = np.zeros(nq, np.int32)
        _check(lib().qadc_query_scan_collect(self._h, slot, _p(keys, u32p), _p(vals, i8p), _p(sizes, i32p),
                                             _p(status, i32p), None, None, None))
        return dict(keys=keys, values=vals, sizes=sizes, status=status)

    def collect_candidates(self, slot, capacity=1 << 18):
        nq, R, tables, assign = self._pending.pop(slot)
        bufs = getattr(self, "_cand_bufs", None)
        u16p = C.POINTER(C.c_uint16)
        if bufs is None or len(bufs[0]) < capacity:        # reused across calls: no per-step page faults
            bufs = self._cand_bufs = (np.zeros(capacity, np.uint32), np.zeros(capacity, np.int8),
                                      np.zeros(capacity, np.uint16))
        ck, cv, cs_ = bufs
        off = np.zeros(nq + 1, np.uint64)
        status = np.zeros(nq, np.int32)
        qmin = np.zeros(nq, np.float32)
        qmax = np.zeros(nq, np.float32)
        rc = lib().qadc_query_scan_collect_candidates(self._h, slot, len(ck), _p(ck, u32p), _p(cv, i8p), _p(cs_, u16p),
                                                      _p(off, u64p), _p(status, i32p), _p(qmin, f32p), _p(qmax, f32p))
        if rc == -3:                                        # QADC_E_CAPACITY: the result is kept, retry larger
            need = int(off[nq]) + 1024
            ck, cv, cs_ = self._cand_bufs = (np.zeros(need, np.uint32), np.zeros(need, np.int8), np.zeros(need, np.uint16))
            rc = lib().qadc_query_scan_collect_candidates(self._h, slot, need, _p(ck, u32p), _p(cv, i8p), _p(cs_, u16p),
                                                          _p(off, u64p), _p(status, i32p), _p(qmin, f32p), _p(qmax, f32p))
        _check(rc)
        return dict(keys=ck, vals=cv, slots=cs_, offsets=off.astype(np.int64), status=status, qmin=qmin, qmax=qmax)

    # ---- native multi-GPU merge (RCCL inside the library) ----------------------------------
    def dist_init(self, rank, world, unique_id):
        uid = np.ascontiguousarray(unique_id, np.uint8)
        assert uid.size == 128
        _check(lib().qadc_dist_init(self._h, rank, world, _p(uid, u8p)))
        self._dist_world = world

    def dist_init_transport(self, transport):
        """The merge over the library's shared-memory transport (ShmTransport) instead of RCCL."""
        fn = C.cast(lib().qadc_shm_transport_allgather, C.c_void_p)
        _check(lib().qadc_dist_init_transport(self._h, transport.rank, transport.world, fn, transport._ctx))
        self._dist_world = transport.world
        self._transport = transport

    def dist_init_loopback(self, rank, world):
        """Measurement aid: this process stands in for rank `rank` of `world` (qadc_dist_init_loopback)."""
        _check(lib().qadc_dist_init_loopback(self._h, rank, world))
        self._dist_world = world

    def dist_shutdown(self):
        _check(lib().qadc_dist_shutdown(self._h))

    def slot_qtables(self, slot, q_first, q_count, ma):
        """int8 tables [q_count][ma][M][16] of the batch last collected from `slot` (qadc_slot_qtables)."""
        out = np.zeros((q_count, ma, self.M, 16), np.int8)
        _check(lib().qadc_slot_qtables(self._h, slot, q_first, q_count, _p(out, i8p)))
        return out

    def slot_assign(self, slot, nq, ma):
        out = np.zeros((nq, ma), np.int32)
        _check(lib().qadc_slot_assign(self._h, slot, _p(out, i32p)))
        return out

    def dist_collect(self, slot, extra=None):
        """Replaces collect(): one ncclAllGather of the ranks' push streams + device-side replay in global scan order.
        Returns dict(keys, values, sizes, status[, extra = float32 [world][n]])."""
        if slot in getattr(self, "_spending", {}):          # a search_submit batch (queries in)
            q, _, R = self._spending.pop(slot)
            nq = q.shape[0]
        else:
            nq, R, tables, assign = self._pending.pop(slot)
        keys = np.zeros((nq, R), np.uint32)
        vals = np.zeros((nq, R), np.int8)
        sizes = np.zeros(nq, np.int32)
        status = np.zeros(nq, np.int32)
        ex = None if extra is None else np.ascontiguousarray(extra, np.float32).reshape(-1)
        world = getattr(self, "_dist_world", 1)
        ex_out = None if ex is None else np.zeros((world, ex.size), np.float32)
        _check(lib().qadc_dist_collect(self._h, slot, _p(keys, u32p), _p(vals, i8p), _p(sizes, i32p), _p(status, i32p),
                                       _p(ex, f32p), 0 if ex is None else ex.size, _p(ex_out, f32p)))
        out = dict(keys=keys, values=vals, sizes=sizes, status=status)
        if ex is not None:
            out["extra"] = ex_out
        return out

    def set_pq(self, codebooks):
        cb = np.ascontiguousarray(codebooks, np.float32)
        assert cb.shape[0] == self.M and cb.shape[1] == 16
        self.dim = self.M * cb.shape[2]
        _check(lib().qadc_index_set_pq(self._h, self.dim, _p(cb, f32p)))

    def set_rotation(self, rotation):
        r = None if rotation is None else np.ascontiguousarray(rotation, np.float32)
        _check(lib().qadc_index_set_rotation(self._h, _p(r, f32p)))

    def set_coarse(self, centroids):
        c = np.ascontiguousarray(centroids, np.float32)
        _check(lib().qadc_index_set_coarse(self._h, c.shape[0], _p(c, f32p)))

    def reconstruct(self, keys):
        """The approximate vectors behind keys of this 4-bit index -> (vectors float32 [n][dim], where uint64 [n]), as
        AdcIndex.reconstruct: a float-ADC view of the index is made, asked, and destroyed.  Needs a finalized index (a view does)
        with set_pq called."""
        view = AdcIndex.view_of(self)
        try:
            return view.reconstruct(keys)
        finally:
            view.close()

    def search(self, queries, ma, R):
        q = np.ascontiguousarray(queries, np.float32)
        nq = q.shape[0]
        keys = np.zeros((nq, R), np.uint32)
        vals = np.zeros((nq, R), np.int8)
        sizes = np.zeros(nq, np.int32)
        status = np.zeros(nq, np.int32)
        assign = np.zeros((nq, ma), np.int32)
        _check(lib().qadc_search(self._h, nq, _p(q, f32p), ma, R, _p(keys, u32p), _p(vals, i8p), _p(sizes, i32p),
                                 _p(status, i32p), _p(assign, i32p)))
        return dict(heaps=self._heaps(nq, R, keys, vals, sizes), status=status, assign=assign, keys=keys,
                    values=vals, sizes=sizes)

    def search_refined(self, queries, ma, R, r_in, store):
        """search(queries, ma, r_in), then the heaps' keys re-ranked by their exact L2 distance to the vectors of the Refine `store`
        -> (keys [nq][R], dist [nq][R], sizes [nq], missing), ascending by (distance, key).  Only the sizes[q] entries a heap holds are
        candidates; a (0, 127) sentinel left among them is key 0, judged by its true distance like any other, once."""
        q = np.ascontiguousarray(queries, np.float32)
        got = self.search(q, ma, r_in)
        return store.rerank(q, got["keys"], R, counts=got["sizes"])

    def search_exact(self, queries, ma, R, store, sum_mode=1, filter=None):
        """AdcIndex.search_exact through a view of this (finalized) index: the exact nearest rows of the Refine `store` among the
        partitions the queries probe -> (keys, dist, sizes, missing, assign)."""
        view = AdcIndex.view_of(self)
        try:
            return view.search_exact(queries, ma, R, store, sum_mode=sum_mode, filter=filter)
        finally:
            view.close()

    def search_submit(self, slot, queries, ma, R):
        """Asynchronous (slot 0..3) form of search(): enqueue a batch, collect it later (overlaps the host replay of
        one batch with the GPU work of the next)."""
        q = np.ascontiguousarray(queries, np.float32)
        self._spending = getattr(self, "_spending", {})
        self._spending[slot] = (q, ma, R)
        _check(lib().qadc_search_submit(self._h, slot, q.shape[0], _p(q, f32p), ma, R))

    def search_collect(self, slot):
        q, ma, R = self._spending.pop(slot)
        nq = q.shape[0]
        keys = np.zeros((nq, R), np.uint32)
        vals = np.zeros((nq, R), np.int8)
        sizes = np.zeros(nq, np.int32)
        status = np.zeros(nq, np.int32)
        assign = np.zeros((nq, ma), np.int32)
        _check(lib().qadc_search_collect(self._h, slot, _p(keys, u32p), _p(vals, i8p), _p(sizes, i32p), _p(status, i32p),
                                         _p(assign, i32p)))
        return dict(keys=keys, values=vals, sizes=sizes, status=status, assign=assign)

    def scan_i8(self, assign, qtables, R):
        assign = self._prep(assign)
        nq, ma = assign.shape
        qt = np.ascontiguousarray(qtables, np.int8)
        assert qt.size == nq * ma * self.M * 16
        keys = np.zeros((nq, R), np.uint32)
        vals = np.zeros((nq, R), np.int8)
        sizes = np.zeros(nq, np.int32)
        _check(lib().qadc_scan_i8(self._h, nq, ma, _p(assign, i32p), _p(qt, i8p), R, _p(keys, u32p), _p(vals, i8p),
                                  _p(sizes, i32p)))
        return self._heaps(nq, R, keys, vals, sizes)

    def scan_i8_candidates(self, assign, qtables, R, capacity=1 << 20):
        assign = self._prep(assign)
        nq, ma = assign.shape
        qt = np.ascontiguousarray(qtables, np.int8)
        ck = np.zeros(capacity, np.uint32)
        cv = np.zeros(capacity, np.int8)
        off = np.zeros(nq + 1, np.uint64)
        _check(lib().qadc_scan_i8_candidates(self._h, nq, ma, _p(assign, i32p), _p(qt, i8p), R, capacity,
                                             _p(ck, u32p), _p(cv, i8p), _p(off, u64p)))
        return [(ck[int(off[q]):int(off[q + 1])].copy(), cv[int(off[q]):int(off[q + 1])].copy()) for q in range(nq)]

    def query_scan_shard_streams(self, assign, tables, R, capacity=1 << 18):
        """submit + collect_candidates: this rank's ordered streams with assign slots (multi-GPU callers)."""
        self.submit(0, assign, tables, R)
        res = self.collect_candidates(0, capacity)
        total = int(res["offsets"][-1])
        return dict(keys=res["keys"][:total].copy(), vals=res["vals"][:total].copy(), slots=res["slots"][:total].copy(),
                    offsets=res["offsets"].copy(), status=res["status"], qmin=res["qmin"], qmax=res["qmax"])

    def query_scan_candidates(self, assign, tables, R, capacity=1 << 20):
        assign = self._prep(assign)
        nq, ma = assign.shape
        ck = np.zeros(capacity, np.uint32)
        cv = np.zeros(capacity, np.int8)
        off = np.zeros(nq + 1, np.uint64)
        status = np.zeros(nq, np.int32)
        qmin = np.zeros(nq, np.float32)
        qmax = np.zeros(nq, np.float32)
        _check(lib().qadc_query_scan_candidates(self._h, nq, ma, _p(assign, i32p), _p(tables, f32p), R, capacity,
                                                _p(ck, u32p), _p(cv, i8p), _p(off, u64p), _p(status, i32p),
                                                _p(qmin, f32p), _p(qmax, f32p)))
        streams = [(ck[int(off[q]):int(off[q + 1])].copy(), cv[int(off[q]):int(off[q + 1])].copy())
                   for q in range(nq)]
        return dict(streams=streams, status=status, qmin=qmin, qmax=qmax)

    def scan_start(self, assign, tables, R):
        assign = self._prep(assign)
        nq, ma = assign.shape
        tb = np.ascontiguousarray(tables, np.float32)
        qmax = np.zeros(nq, np.float32)
        _check(lib().qadc_scan_start(self._h, nq, ma, _p(assign, i32p), _p(tb, f32p), R, _p(qmax, f32p)))
        return qmax

    def candidates_i8(self, part, qtable):
        qt = np.ascontiguousarray(qtable, np.int8)
        out = np.zeros(self.partition_size(part), np.int8)
        _check(lib().qadc_candidates_i8(self._h, part, _p(qt, i8p), _p(out, i8p)))
        return out

    def float_top1(self, part, table):
        tb = np.ascontiguousarray(table, np.float32).reshape(-1)
        key, pos, dist = C.c_uint32(0), C.c_uint32(0), C.c_float(0)
        _check(lib().qadc_float_top1(self._h, part, _p(tb, f32p), C.byref(key), C.byref(pos), C.byref(dist)))
        return key.value, pos.value, dist.value

    def profile(self):
        pr = Profile()
        _check(lib().qadc_profile_read(self._h, C.byref(pr)))
        return {f: getattr(pr, f) for f, _ in Profile._fields_}

    def profile_reset(self):
        _check(lib().qadc_profile_reset(self._h))


QADC_ADC_FILTER_EXCLUDE, QADC_ADC_FILTER_ALLOW = 0, 1   # include/qadc.h
_FILTER_MODES = {"exclude": QADC_ADC_FILTER_EXCLUDE, "allow": QADC_ADC_FILTER_ALLOW}


class AdcFilter:
    """A key set for AdcIndex.set_filter (qadc_adc_filter_create): mode "exclude" drops the rows whose key is in `keys`, "allow" the
    rows whose key is not.  A row's key is its label, else its position (+ a view's key_base).  Immutable; may be set on several
    indexes of its device; close() raises QadcError while it is set on one."""

    def __init__(self, keys, mode="exclude", device=0):
        k = np.ascontiguousarray(np.asarray(keys, np.uint32).reshape(-1))
        self._create(lambda h: lib().qadc_adc_filter_create(h, self._mode(mode), _p(k, u32p), k.size, device), device)

    @classmethod
    def from_device(cls, keys, mode="exclude"):
        """The set from a contiguous 1-d int32 torch tensor that carries the keys' uint32 bits — the form in which search_device
        returns keys — read where it lies; the filter is on the tensor's device."""
        import torch
        if not isinstance(keys, torch.Tensor):
            raise TypeError("keys must be a torch.Tensor, not %s" % type(keys).__name__)
        if keys.device.type != "cuda":
            raise QadcError("keys is on %s, not on a GPU" % keys.device)
        device = keys.device.index
        t = _label_tensor(keys, device)
        self = cls.__new__(cls)
        self._create(lambda h: lib().qadc_adc_filter_create_device(h, cls._mode(mode), t.data_ptr(), int(t.shape[0]), device), device)
        return self

    @classmethod
    def create_raw(cls, mode, keys, count, device=0):
        """The C call as it is (mode: an int; keys: a uint32 array or None)."""
        self = cls.__new__(cls)
        self._create(lambda h: lib().qadc_adc_filter_create(h, mode, _p(keys, u32p), count, device), device)
        return self

    @staticmethod
    def _mode(mode):
        if mode not in _FILTER_MODES:
            raise ValueError('mode is "exclude" or "allow", not %r' % (mode,))
        return _FILTER_MODES[mode]

    def _create(self, call, device):
        self._h = C.c_void_p()
        self.device = device
        _check(call(C.byref(self._h)))

    def info(self):
        """-> dict(mode "exclude" | "allow", lo, hi: the smallest and largest key (an empty set: lo 2^32 - 1, hi 0), bitmap_bytes)"""
        mode, lo, hi, nbytes = C.c_int(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        _check(lib().qadc_adc_filter_info(self._h, C.byref(mode), C.byref(lo), C.byref(hi), C.byref(nbytes)))
        return dict(mode="allow" if mode.value == QADC_ADC_FILTER_ALLOW else "exclude", lo=int(lo.value), hi=int(hi.value),
                    bitmap_bytes=int(nbytes.value))

    def close(self):
        """qadc_adc_filter_destroy: raises QadcError (QADC_E_STATE) while the filter is set on an index"""
        if getattr(self, "_h", None):
            _check(lib().qadc_adc_filter_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AdcIndex(_RowStoreMixin):
    """One GPU-resident PQ database with whole-byte codes, scanned with float tables: the role of the reference's
    scanner_simple after prepare_database (db_query.cpp:17-46).  sq_bits 8 with sq_count 4, 8 or 16.
    AdcIndex.create16(sq_count): 16-bit sub-quantizers, sq_count 2, 4 or 8 (scan_standard<uint16_t, NSQ>).
    AdcIndex.view_of(index): the same front end on the 4-bit codes of an Index, read in place (scan_4<M>)."""

    centroids = 256                                                      # per sub-quantizer (create16: 65536; a view: 16)

    def __init__(self, sq_count, sq_bits, device=0):
        self.sq_count = sq_count
        self.table_dim = sq_count * 256                                  # floats of one (query, probe) table
        self.device = device
        self._source = None
        self._h = C.c_void_p()
        _check(lib().qadc_adc_index_create(C.byref(self._h), sq_count, sq_bits, device))

    @classmethod
    def create16(cls, sq_count, device=0):
        """qadc_adc_index_create16: an index of its own over 16-bit codes, sq_count 2, 4 or 8 with 65536 centroids each: codes
        uint16 [n][sq_count] (or their little-endian bytes, uint8 [n][2*sq_count]), tables [nq][ma][sq_count*65536], codebooks
        [sq_count][65536][dim/sq_count].  Every method of an AdcIndex works on it."""
        self = cls.__new__(cls)
        self.sq_count = sq_count
        self.centroids = 65536
        self.table_dim = sq_count * 65536
        self.device = device
        self._source = None
        self._h = C.c_void_p()
        _check(lib().qadc_adc_index_create16(C.byref(self._h), sq_count, device))
        return self

    @classmethod
    def view_of(cls, index):
        """qadc_adc_index_create_view: an AdcIndex on the partitions of the finalized pyqadc.Index `index`, on its device, M
        sub-quantizers of 4 bits, tables [nq][ma][M*16].  It copies nothing and keeps `index` referenced;
        index.close() raises until the view is closed.  The search calls run the quantizers set on `index`."""
        self = cls.__new__(cls)
        self.sq_count = index.M
        self.centroids = 16
        self.table_dim = index.M * 16
        self.device = index.device
        self._source = None
        self._h = C.c_void_p()
        _check(lib().qadc_adc_index_create_view(C.byref(self._h), index._h))
        self._source = index                                             # (collected after the view: __del__ closes the view first)
        return self

    @property
    def dim(self):
        """the vector dimension: set_pq's, or for a view the one set on its source index (AttributeError before either)"""
        if self._source is not None:
            return self._source.dim
        try:
            return self.__dict__["_dim"]
        except KeyError:
            raise AttributeError("dim") from None

    @dim.setter
    def dim(self, value):
        self.__dict__["_dim"] = value

    def close(self):
        if self._h:
            lib().qadc_adc_index_destroy(self._h)
            self._h = C.c_void_p()
        self._source = None
        self._filter = None

    def set_filter(self, f):
        """qadc_adc_index_set_filter: every later query_scan* / search* call drops the rows whose key does not pass the AdcFilter `f`;
        None clears it.  The index keeps `f` referenced while it is set."""
        if f is not None and not isinstance(f, AdcFilter):
            raise TypeError("set_filter takes an AdcFilter or None, not %s" % type(f).__name__)
        _check(lib().qadc_adc_index_set_filter(self._h, None if f is None else f._h))
        self._filter = f

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _filters(self, filters, nq):
        """filters= of a scanning call -> the array the *_filtered C call takes, or None (the plain call): a sequence of nq
        AdcFilter | None.  ValueError: another length; TypeError: an entry of another type; QadcError: a closed filter."""
        if filters is None:
            return None
        filters = list(filters)
        if len(filters) != nq:
            raise ValueError("filters has %d entries for %d queries" % (len(filters), nq))
        arr = (C.c_void_p * nq)()
        for q, f in enumerate(filters):
            if f is None:
                continue
            if not isinstance(f, AdcFilter):
                raise TypeError("filters[%d] is %s, not an AdcFilter or None" % (q, type(f).__name__))
            if not getattr(f, "_h", None):
                raise QadcError("filters[%d] is closed" % q)
            arr[q] = f._h.value
        return arr

    def _scan_call(self, name, filters, *args):
        """the plain C call, or with a filters array its _filtered form"""
        if filters is None:
            return getattr(lib(), name)(*args)
        return getattr(lib(), name + "_filtered")(*args, filters)

    def _code_rows(self, c):
        """one partition's codes as the bytes the C call takes: uint8 [n][code bytes]"""
        if self.centroids != 65536:
            return np.ascontiguousarray(c, np.uint8).reshape(-1, self.sq_count)
        c = np.asarray(c)
        if c.dtype != np.uint8:                                          # uint16 [n][sq_count] -> little-endian bytes
            if c.dtype.kind not in "ui" or (c.size and (int(c.min()) < 0 or int(c.max()) > 0xffff)):
                raise QadcError("16-bit codes are uint16 [n][sq_count] or uint8 [n][2*sq_count]")
            c = np.ascontiguousarray(c.reshape(-1, self.sq_count).astype("<u2")).view(np.uint8)
        return np.ascontiguousarray(c, np.uint8).reshape(-1, 2 * self.sq_count)

    def add_partitions(self, codes, labels=None):
        """codes: one array per partition, uint8 [n][sq_count] (a create16 index: uint16 [n][sq_count] or uint8 [n][2*sq_count])"""
        codes = [self._code_rows(c) for c in codes]
        sizes = np.array([c.shape[0] for c in codes], np.uint32)
        ca = (u8p * len(codes))(*[_p(c, u8p) for c in codes])
        la = None
        if labels is not None:
            labels = [None if l is None else np.ascontiguousarray(l, np.uint32) for l in labels]
            la = (u32p * len(labels))(*[None if l is None else _p(l, u32p) for l in labels])
        _check(lib().qadc_adc_index_add_partitions(self._h, len(codes), ca, la, _p(sizes, u32p)))

    def partition_count(self):
        return lib().qadc_adc_index_partition_count(self._h)

    def partition_size(self, part):
        return lib().qadc_adc_index_partition_size(self._h, part)

    # ---- db_add and remove by label (qadc_adc_index_add_vectors*, _reserve, _read_partition, _remove_labels*): _RowStoreMixin ----
    _c_prefix = "qadc_adc_index_"

    def _row_format(self):
        return self.sq_count, ("<u2" if self.centroids == 65536 else np.uint8)

    def _device_vectors(self, vectors):
        if getattr(vectors, "ndim", 0) != 2:
            raise TypeError("vectors must be a 2-d torch.Tensor")
        return self._device_tensor(vectors, (int(vectors.shape[0]), getattr(self, "dim", int(vectors.shape[1]))), "vectors")

    def reruns(self):
        """query calls on this index that were re-run because a candidate region overflowed"""
        return lib().qadc_adc_index_reruns(self._h)

    def set_finish(self, mode):
        """0 (default): the host orders the kept candidates and replays the heaps; 1: query_scan and search do both on the GPU and
        fetch only the heaps' arrays (same arrays, bit for bit)"""
        _check(lib().qadc_adc_index_set_finish(self._h, int(mode)))

    def host_finishes(self):
        """queries finished on the host while the device finish was asked for (R > 4096 is the only cause)"""
        return lib().qadc_adc_index_host_finishes(self._h)

    def _inputs(self, assign, tables):
        assign = np.ascontiguousarray(assign, np.int32)
        if assign.ndim == 1:
            assign = assign.reshape(1, -1)
        nq, ma = assign.shape
        tables = np.ascontiguousarray(tables, np.float32).reshape(nq, ma, self.table_dim)
        return assign, tables, nq, ma

    def query_scan(self, assign, tables, R, sum_mode=1, filters=None):
        """assign [nq][ma], tables [nq][ma][table_dim] (sq_count*256; create16: sq_count*65536; a view: sq_count*16) -> (keys [nq][R], vals [nq][R], sizes [nq]): the heap arrays
        of scanner_simple::query_scan per query (rows are valid up to sizes[q]).  filters: None, or a sequence of nq AdcFilter | None,
        the filter of each query (qadc_adc_query_scan_filtered): query q also drops the rows whose key does not pass filters[q]."""
        assign, tables, nq, ma = self._inputs(assign, tables)
        fl = self._filters(filters, nq)
        keys = np.zeros((nq, R), np.uint32)
        vals = np.zeros((nq, R), np.float32)
        sizes = np.zeros(nq, np.int32)
        _check(self._scan_call("qadc_adc_query_scan", fl, self._h, nq, ma, _p(assign, i32p), _p(tables, f32p), R, sum_mode, _p(keys, u32p),
                               _p(vals, f32p), _p(sizes, i32p)))
        return keys, vals, sizes

    def query_scan_candidates(self, assign, tables, R, sum_mode=1, capacity=None, filters=None):
        """-> (keys, vals, offsets [nq+1]): the ordered candidate stream (query q = [offsets[q], offsets[q+1])), to be pushed
        after the R sentinels.  capacity=None sizes the buffers itself; a given capacity that is too small raises QadcError
        (offsets[nq] then holds the entries needed: see query_scan_candidates_raw).  filters: as query_scan's."""
        if capacity is not None:
            rc, keys, vals, offsets = self.query_scan_candidates_raw(assign, tables, R, sum_mode, capacity, filters)
            _check(rc)
            return keys, vals, offsets
        cap = 1 << 16
        while True:
            rc, keys, vals, offsets = self.query_scan_candidates_raw(assign, tables, R, sum_mode, cap, filters)
            if rc != QADC_E_CAPACITY:
                _check(rc)
                return keys[:offsets[-1]], vals[:offsets[-1]], offsets
            cap = int(offsets[-1])

    def query_scan_candidates_raw(self, assign, tables, R, sum_mode, capacity, filters=None):
        """The C call as it is: -> (rc, keys [capacity], vals [capacity], offsets [nq+1])."""
        assign, tables, nq, ma = self._inputs(assign, tables)
        fl = self._filters(filters, nq)
        keys = np.zeros(max(capacity, 1), np.uint32)
        vals = np.zeros(max(capacity, 1), np.float32)
        offsets = np.zeros(nq + 1, np.uint64)
        rc = self._scan_call("qadc_adc_query_scan_candidates", fl, self._h, nq, ma, _p(assign, i32p), _p(tables, f32p), R, sum_mode,
                             capacity, _p(keys, u32p), _p(vals, f32p), _p(offsets, u64p))
        return rc, keys, vals, offsets

    # ---- from query vectors: the feeders run on the GPU (qadc_adc_search*) ----
    def set_pq(self, codebooks):
        """codebooks [sq_count][256][dim / sq_count] (a create16 index: [sq_count][65536][dim / sq_count])"""
        cb = np.ascontiguousarray(codebooks, np.float32)
        assert cb.ndim == 3 and cb.shape[0] == self.sq_count and cb.shape[1] == self.centroids
        self.set_pq_raw(self.sq_count * cb.shape[2], cb)

    def set_pq_raw(self, dim, codebooks):
        """The C call as it is (any dim: a bad one raises QadcError)."""
        cb = np.ascontiguousarray(codebooks, np.float32)
        _check(lib().qadc_adc_index_set_pq(self._h, dim, _p(cb, f32p)))
        self.dim = dim

    def set_rotation(self, rotation):
        r = None if rotation is None else np.ascontiguousarray(rotation, np.float32)
        dim = getattr(self, "dim", None)
        assert r is None or dim is None or r.shape == (dim, dim)
        _check(lib().qadc_adc_index_set_rotation(self._h, _p(r, f32p)))

    def set_coarse(self, centroids):
        """centroids [K][dim]; None = a flat index"""
        if centroids is None:
            _check(lib().qadc_adc_index_set_coarse(self._h, 0, None))
            return
        c = np.ascontiguousarray(centroids, np.float32)
        assert c.ndim == 2 and c.shape[1] == getattr(self, "dim", c.shape[1])
        _check(lib().qadc_adc_index_set_coarse(self._h, c.shape[0], _p(c, f32p)))

    def set_table_budget(self, nbytes):
        """device memory for the tables of one pass (0 = the default, 1 GiB); larger batches run in sub-batches of whole queries"""
        _check(lib().qadc_adc_index_set_table_budget(self._h, int(nbytes)))

    def _queries(self, queries):
        q = np.ascontiguousarray(queries, np.float32)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        assert q.ndim == 2 and q.shape[1] == getattr(self, "dim", q.shape[1])
        return q

    def search(self, queries, ma, R, table_form=2, sum_mode=1, filters=None):
        """queries [nq][dim] -> (keys [nq][R], vals [nq][R], sizes [nq], assign [nq][ma]): query_scan's heap arrays on tables
        built on the GPU.  table_form 0 = direct, 1 = BLAS expansion, 2 = nns_engine's rule (direct iff ma == 1).  filters: None, or
        a sequence of nq AdcFilter | None, the filter of each query (qadc_adc_search_filtered), on top of set_filter's."""
        q = self._queries(queries)
        nq = q.shape[0]
        fl = self._filters(filters, nq)
        keys = np.zeros((nq, R), np.uint32)
        vals = np.zeros((nq, R), np.float32)
        sizes = np.zeros(nq, np.int32)
        assign = np.zeros((nq, ma), np.int32)
        _check(self._scan_call("qadc_adc_search", fl, self._h, nq, _p(q, f32p), ma, R, table_form, sum_mode, _p(keys, u32p), _p(vals, f32p),
                               _p(sizes, i32p), _p(assign, i32p)))
        return keys, vals, sizes, assign

    def search_refined(self, queries, ma, R, r_in, store, table_form=2, sum_mode=1, filters=None):
        """search(queries, ma, r_in), then the heaps' keys re-ranked by their exact L2 distance to the vectors of the Refine `store`
        -> (keys [nq][R], dist [nq][R], sizes [nq], missing), ascending by (distance, key).  The heaps' FLT_MAX sentinels are no
        candidates; a filter set on the index, and the filters= of the queries, hold for the refined keys, which are a subset of the
        heaps'."""
        q = self._queries(queries)
        keys, vals, _, _ = self.search(q, ma, r_in, table_form, sum_mode, filters=filters)
        return store.rerank(q, keys, R, values=vals)

    def search_refined_device(self, queries, ma, R, r_in, store, table_form=2, sum_mode=1, filters=None):
        """search_device, then store.rerank_device on its tensors: queries in device memory in, (keys int32 [nq][R] carrying the
        uint32 bits, dist float32 [nq][R], sizes int32 [nq]) in device memory out, and the missing count; nothing else crosses the bus."""
        keys, vals, _ = self.search_device(queries, ma, r_in, table_form, sum_mode, filters=filters)
        return store.rerank_device(queries, keys, R, values=vals)

    # ---- the coarse step alone, and exact search over the probed partitions (qadc_adc_index_assign*, qadc_adc_search_exact*;
    # DESIGN.md section 11.22) ----
    def assign(self, queries, ma, sum_mode=1):
        """queries [nq][dim] -> assign int32 [nq][ma]: the probe lists search() reports (all zero on an index without coarse centroids)"""
        q = self._queries(queries)
        assign = np.zeros((q.shape[0], ma), np.int32)
        _check(lib().qadc_adc_index_assign(self._h, q.shape[0], _p(q, f32p), ma, sum_mode, _p(assign, i32p)))
        return assign

    def assign_device(self, queries, ma, sum_mode=1):
        """assign() on a float32 tensor [nq][dim] of the index's device -> an int32 tensor [nq][ma] on that device"""
        import torch
        if getattr(queries, "ndim", 0) != 2:
            raise TypeError("queries must be a 2-d torch.Tensor")
        nq = int(queries.shape[0])
        q = self._device_tensor(queries, (nq, getattr(self, "dim", int(queries.shape[1]))), "queries")
        dev = torch.device("cuda", self.device)
        assign = torch.zeros((nq, int(ma)), dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        _check(lib().qadc_adc_index_assign_device(self._h, nq, q.data_ptr(), ma, sum_mode, assign.data_ptr()))
        return assign

    def search_exact(self, queries, ma, R, store, sum_mode=1, filter=None):
        """assign(queries, ma), then store.knn_probed on its lists -> (keys uint32 [nq][R], dist float32 [nq][R], sizes [nq], missing,
        assign [nq][ma]): the exact nearest rows among the partitions search() would probe — the ceiling of search_refined at the same
        ma.  filter: an AdcFilter or None, on top of set_filter's."""
        q = self._queries(queries)
        nq, R = q.shape[0], int(R)
        ok = np.zeros((nq, R), np.uint32)
        od = np.zeros((nq, R), np.float32)
        osz = np.zeros(nq, np.int32)
        assign = np.zeros((nq, ma), np.int32)
        missing = C.c_uint64(0)
        _check(lib().qadc_adc_search_exact(self._h, store._h, nq, _p(q, f32p), ma, R, sum_mode, None if filter is None else filter._h,
                                           _p(ok, u32p), _p(od, f32p), _p(osz, i32p), C.byref(missing), _p(assign, i32p)))
        return ok, od, osz, int(missing.value), assign

    def search_exact_device(self, queries, ma, R, store, sum_mode=1, filter=None):
        """search_exact() on a float32 tensor [nq][dim] of the index's device -> tensors (keys int32 [nq][R] carrying the uint32 bits,
        dist float32 [nq][R], sizes int32 [nq]), missing (an int) and assign (int32 [nq][ma]) on that device"""
        import torch
        if getattr(queries, "ndim", 0) != 2:
            raise TypeError("queries must be a 2-d torch.Tensor")
        nq, R = int(queries.shape[0]), int(R)
        q = self._device_tensor(queries, (nq, getattr(self, "dim", int(queries.shape[1]))), "queries")
        keys, dist, sizes = self._device_outputs(nq, R)
        dev = torch.device("cuda", self.device)
        assign = torch.zeros((nq, int(ma)), dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        missing = C.c_uint64(0)
        _check(lib().qadc_adc_search_exact_device(self._h, store._h, nq, q.data_ptr(), ma, R, sum_mode, None if filter is None else filter._h,
                                                  keys.data_ptr(), dist.data_ptr(), sizes.data_ptr(), C.byref(missing), assign.data_ptr()))
        return keys, dist, sizes, int(missing.value), assign

    def search_candidates(self, queries, ma, R, table_form=2, sum_mode=1, filters=None):
        """-> (keys, vals, offsets [nq+1], assign [nq][ma]): the ordered candidate stream, as query_scan_candidates returns it"""
        q = self._queries(queries)
        nq = q.shape[0]
        fl = self._filters(filters, nq)
        assign = np.zeros((nq, ma), np.int32)
        offsets = np.zeros(nq + 1, np.uint64)
        cap = 1 << 16
        while True:
            keys = np.zeros(cap, np.uint32)
            vals = np.zeros(cap, np.float32)
            rc = self._scan_call("qadc_adc_search_candidates", fl, self._h, nq, _p(q, f32p), ma, R, table_form, sum_mode, cap, _p(keys, u32p),
                                 _p(vals, f32p), _p(offsets, u64p), _p(assign, i32p))
            if rc != QADC_E_CAPACITY:
                _check(rc)
                return keys[:offsets[-1]], vals[:offsets[-1]], offsets, assign
            cap = int(offsets[-1])

    def search_tables(self, queries, ma, table_form=2, sum_mode=1):
        """The feeders alone -> (assign [nq][ma], tables [nq][ma][table_dim])"""
        q = self._queries(queries)
        nq = q.shape[0]
        assign = np.zeros((nq, ma), np.int32)
        tables = np.zeros((nq, ma, self.table_dim), np.float32)
        _check(lib().qadc_adc_search_tables(self._h, nq, _p(q, f32p), ma, table_form, sum_mode, _p(assign, i32p), _p(tables, f32p)))
        return assign, tables

    # ---- device memory in, device memory out: torch tensors by data_ptr() (torch is imported here only) ----
    def _device_tensor(self, t, shape, what):
        import torch
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor, not %s" % (what, type(t).__name__))
        if t.dtype != torch.float32:
            raise TypeError("%s must be float32, not %s" % (what, t.dtype))
        if t.device.type != "cuda" or t.device.index != self.device:
            raise QadcError("%s is on %s; the index is on device %d" % (what, t.device, self.device))
        if not t.is_contiguous():
            raise QadcError("%s must be contiguous" % what)
        if tuple(t.shape) != tuple(shape):
            raise QadcError("%s has shape %s, expected %s" % (what, tuple(t.shape), tuple(shape)))
        return t

    def _device_outputs(self, nq, R):
        import torch
        dev = torch.device("cuda", self.device)
        keys = torch.zeros((nq, R), dtype=torch.int32, device=dev)       # the uint32 keys' bits
        vals = torch.zeros((nq, R), dtype=torch.float32, device=dev)
        sizes = torch.zeros((nq,), dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()                     # inputs and the zero fills are complete before the call
        return keys, vals, sizes

    def search_device(self, queries, ma, R, table_form=2, sum_mode=1, filters=None):
        """queries: float32 tensor [nq][dim] on the index's device -> tensors (keys int32 [nq][R] carrying the uint32 bits,
        vals float32 [nq][R], sizes int32 [nq]) on that device: search()'s heap arrays, finished on the GPU; no host copy."""
        if getattr(queries, "ndim", 0) != 2:
            raise TypeError("queries must be a 2-d torch.Tensor")
        nq = int(queries.shape[0])
        q = self._device_tensor(queries, (nq, getattr(self, "dim", int(queries.shape[1]))), "queries")
        fl = self._filters(filters, nq)                                  # (host memory: AdcFilter | None per query, as search's)
        keys, vals, sizes = self._device_outputs(nq, int(R))
        _check(self._scan_call("qadc_adc_search_device", fl, self._h, nq, q.data_ptr(), ma, R, table_form, sum_mode, keys.data_ptr(),
                               vals.data_ptr(), sizes.data_ptr()))
        return keys, vals, sizes

    def query_scan_device(self, assign, tables, R, sum_mode=1, filters=None):
        """assign [nq][ma] (host), tables: float32 tensor [nq][ma][table_dim] on the index's device -> tensors (keys, vals,
        sizes) as search_device: query_scan()'s heap arrays without the upload of the tables."""
        assign = np.ascontiguousarray(assign, np.int32)
        if assign.ndim == 1:
            assign = assign.reshape(1, -1)
        nq, ma = assign.shape
        t = self._device_tensor(tables, (nq, ma, self.table_dim), "tables")
        fl = self._filters(filters, nq)
        keys, vals, sizes = self._device_outputs(nq, int(R))
        _check(self._scan_call("qadc_adc_query_scan_device", fl, self._h, nq, ma, _p(assign, i32p), t.data_ptr(), R, sum_mode, keys.data_ptr(),
                               vals.data_ptr(), sizes.data_ptr()))
        return keys, vals, sizes

    # ---- reconstruction: stored codes back to vectors (qadc_adc_index_reconstruct*) ----
    def reconstruct(self, keys):
        """keys (anything np.asarray(..., np.uint32) accepts; what search returns) -> (vectors float32 [n][dim], where uint64 [n]):
        the approximate vector behind each key under the quantizers the index holds now, and (partition << 32 | row) of the row
        taken — the smallest (partition, row) where several rows hold the key.  A key no row holds: a row of NaN (0x7FC00000) and
        where = QADC_RECONSTRUCT_MISSING.  Filters set on the index are ignored."""
        k = np.ascontiguousarray(np.asarray(keys, np.uint32).reshape(-1))
        dim = getattr(self, "dim", 0) or 0
        out = np.zeros((k.size, dim), np.float32)
        where = np.zeros(k.size, np.uint64)
        _check(lib().qadc_adc_index_reconstruct(self._h, _p(k, u32p), k.size, _p(out, f32p), _p(where, u64p)))
        return out, where

    def reconstruct_device(self, keys, out=None):
        """reconstruct for a contiguous int32 torch tensor on the index's device that carries the keys' uint32 bits — any shape, so
        search_device's keys go in unchanged -> (vectors float32 tensor keys.shape + (dim,), where int64 tensor keys.shape carrying
        the uint64 bits: -1 for a missing key) on that device.  out=: a float32 tensor of that shape to write into."""
        import torch
        t = _label_tensor(keys.reshape(-1) if isinstance(keys, torch.Tensor) and keys.is_contiguous() else keys, self.device)
        n, dim = int(t.shape[0]), getattr(self, "dim", 0) or 0
        dev = torch.device("cuda", self.device)
        shape = tuple(keys.shape)
        if out is None:
            out = torch.zeros(shape + (dim,), dtype=torch.float32, device=dev)
        else:
            self._device_tensor(out, shape + (dim,), "out")
        where = torch.zeros(shape, dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()                     # the inputs and the zero fills are complete before the call
        _check(lib().qadc_adc_index_reconstruct_device(self._h, t.data_ptr(), n, out.data_ptr(), where.data_ptr()))
        return out, where

    def reconstruct_rows(self, part, first=0, count=None):
        """rows [first, first + count) of partition `part` (default: all of it) -> vectors float32 [count][dim]; no lookup"""
        if count is None:
            count = max(self.partition_size(part) - first, 0) if 0 <= part < self.partition_count() else 0
        out = np.zeros((count, getattr(self, "dim", 0) or 0), np.float32)
        _check(lib().qadc_adc_index_reconstruct_rows(self._h, part, first, count, _p(out, f32p)))
        return out

    def reconstruct_rows_device(self, part, first, count, out=None):
        """reconstruct_rows into a float32 torch tensor [count][dim] on the index's device"""
        import torch
        dev = torch.device("cuda", self.device)
        dim = getattr(self, "dim", 0) or 0
        if out is None:
            out = torch.zeros((count, dim), dtype=torch.float32, device=dev)
        else:
            self._device_tensor(out, (count, dim), "out")
        torch.cuda.current_stream(dev).synchronize()
        _check(lib().qadc_adc_index_reconstruct_rows_device(self._h, part, first, count, out.data_ptr()))
        return out

    def search_reconstruct(self, queries, ma, R, table_form=2, sum_mode=1, filters=None):
        """search_device, then reconstruct_device on its keys: queries a float32 tensor [nq][dim] on the index's device ->
        (keys, vals, sizes as search_device returns them, vectors float32 tensor [nq][R][dim], where int64 tensor [nq][R]).  The
        slots behind sizes[q] hold no candidate: they are missing rows (NaN, where -1) whatever their key slot holds."""
        import torch
        keys, vals, sizes = self.search_device(queries, ma, R, table_form, sum_mode, filters=filters)
        vectors, where = self.reconstruct_device(keys)
        empty = torch.arange(int(R), device=keys.device).unsqueeze(0) >= sizes.unsqueeze(1)
        nan = torch.tensor([DECODE_NAN_BITS], dtype=torch.int32, device=keys.device).view(torch.float32)
        vectors[empty] = nan
        where[empty] = -1
        return keys, vals, sizes, vectors, where

    # ---- range search: every row below a radius, sorted on the GPU (qadc_adc_range_*) ----
    @staticmethod
    def _radius(radius, nq):
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float32), (nq,)) if np.ndim(radius) == 0 else radius, np.float32)
        if r.shape != (nq,):
            raise ValueError("radius is a scalar or has one entry per query (%d), not shape %s" % (nq, r.shape))
        return r

    def range_collect_raw(self, capacity):
        """The C call as it is: -> (rc, keys [capacity], values [capacity])"""
        keys = np.zeros(max(capacity, 1), np.uint32)
        vals = np.zeros(max(capacity, 1), np.float32)
        return lib().qadc_adc_range_collect(self._h, capacity, _p(keys, u32p), _p(vals, f32p)), keys, vals

    def range_collect(self, lims=None):
        """qadc_adc_range_collect: (keys uint32, values float32) of the range result the index holds, any number of times; lims: the
        array the range call returned (default: the last one made through this object)."""
        n = int(lims[-1]) if lims is not None else getattr(self, "_range_rows", 0)
        rc, keys, vals = self.range_collect_raw(n)
        _check(rc)
        return keys[:n], vals[:n]

    def _range_collect_device(self, lims):
        import torch
        dev = torch.device("cuda", self.device)
        n = int(lims[-1])
        keys = torch.zeros((n,), dtype=torch.int32, device=dev)          # the uint32 keys' bits
        vals = torch.zeros((n,), dtype=torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()                     # the zero fills are complete before the call
        _check(lib().qadc_adc_range_collect_device(self._h, n, keys.data_ptr(), vals.data_ptr()))
        return keys, vals

    def range_scan(self, assign, tables, radius, sum_mode=1, filters=None):
        """assign [nq][ma], tables [nq][ma][table_dim], radius a scalar or [nq] -> (lims int64 [nq+1], keys uint32, values float32): for
        query q, rows [lims[q], lims[q+1]) = every row of its probed partitions whose candidate is < radius[q] (a float compare: NaN keeps
        nothing) and whose key passes set_filter's filter and filters[q], ascending by (candidate, key); scanner_simple::range_scan."""
        assign, tables, nq, ma = self._inputs(assign, tables)
        r = self._radius(radius, nq)
        lims = np.zeros(nq + 1, np.uint64)
        _check(lib().qadc_adc_range_scan(self._h, nq, ma, _p(assign, i32p), _p(tables, f32p), _p(r, f32p), sum_mode, self._filters(filters, nq),
                                         _p(lims, u64p)))
        self._range_rows = int(lims[-1])
        keys, vals = self.range_collect(lims)
        return lims.astype(np.int64), keys, vals

    def range_search(self, queries, ma, radius, table_form=2, sum_mode=1, filters=None):
        """queries [nq][dim] -> (lims, keys, values) as range_scan, on tables built on the GPU as search builds them."""
        q = self._queries(queries)
        nq = q.shape[0]
        r = self._radius(radius, nq)
        lims = np.zeros(nq + 1, np.uint64)
        _check(lib().qadc_adc_range_search(self._h, nq, _p(q, f32p), ma, _p(r, f32p), table_form, sum_mode, self._filters(filters, nq), None,
                                           _p(lims, u64p)))
        self._range_rows = int(lims[-1])
        keys, vals = self.range_collect(lims)
        return lims.astype(np.int64), keys, vals

    def range_scan_device(self, assign, tables, radius, sum_mode=1, filters=None):
        """tables: float32 tensor [nq][ma][table_dim] on the index's device -> (lims int64 [nq+1] numpy, keys int32 tensor carrying the
        uint32 bits, values float32 tensor): range_scan without the upload of the tables or the download of the rows."""
        assign = np.ascontiguousarray(assign, np.int32)
        if assign.ndim == 1:
            assign = assign.reshape(1, -1)
        nq, ma = assign.shape
        t = self._device_tensor(tables, (nq, ma, self.table_dim), "tables")
        r = self._radius(radius, nq)
        lims = np.zeros(nq + 1, np.uint64)
        import torch
        torch.cuda.current_stream(t.device).synchronize()                # the tables are complete before the call
        _check(lib().qadc_adc_range_scan_device(self._h, nq, ma, _p(assign, i32p), t.data_ptr(), _p(r, f32p), sum_mode,
                                                self._filters(filters, nq), _p(lims, u64p)))
        self._range_rows = int(lims[-1])
        keys, vals = self._range_collect_device(lims)
        return lims.astype(np.int64), keys, vals

    def range_search_device(self, queries, ma, radius, table_form=2, sum_mode=1, filters=None):
        """queries: float32 tensor [nq][dim] on the index's device -> (lims numpy, keys tensor, values tensor) as range_scan_device."""
        if getattr(queries, "ndim", 0) != 2:
            raise TypeError("queries must be a 2-d torch.Tensor")
        nq = int(queries.shape[0])
        q = self._device_tensor(queries, (nq, getattr(self, "dim", int(queries.shape[1]))), "queries")
        r = self._radius(radius, nq)
        lims = np.zeros(nq + 1, np.uint64)
        import torch
        torch.cuda.current_stream(q.device).synchronize()                # the queries are complete before the call
        _check(lib().qadc_adc_range_search_device(self._h, nq, q.data_ptr(), ma, _p(r, f32p), table_form, sum_mode, self._filters(filters, nq),
                                                  None, _p(lims, u64p)))
        self._range_rows = int(lims[-1])
        keys, vals = self._range_collect_device(lims)
        return lims.astype(np.int64), keys, vals

    def range_search_refined_device(self, queries, ma, adc_radius, radius, store, table_form=2, sum_mode=1, filters=None):
        """queries: float32 tensor [nq][dim] on the index's device; store: a Refine of that device -> (lims int64 numpy, keys int32
        tensor carrying the uint32 bits, dist float32 tensor, missing): range_search_device under adc_radius, its rows collected in
        device memory and handed to store.rerank_range_device under radius — every key of the ADC result whose exact squared L2
        distance is < radius[q], once, ascending by (distance, key).  Only the two lims arrays and the missing count cross the bus."""
        lims, keys, _ = self.range_search_device(queries, ma, adc_radius, table_form, sum_mode, filters)
        return store.rerank_range_device(queries, lims, keys, radius)

    def range_search_refined(self, queries, ma, adc_radius, radius, store, table_form=2, sum_mode=1, filters=None):
        """the same for host arrays, through range_search and store.rerank_range (the ADC rows cross the bus both ways; the device
        form keeps them where they are): -> (lims int64, keys uint32, dist float32, missing)"""
        q = self._queries(queries)
        lims, keys, _ = self.range_search(q, ma, adc_radius, table_form, sum_mode, filters)
        return store.rerank_range(q, lims, keys, radius)


QADC_REFINE_F32, QADC_REFINE_F16, QADC_REFINE_MAX_IN = 0, 1, 8192   # include/qadc.h
QADC_REFINE_SQ8 = 2
_REFINE_DTYPES = {"f32": QADC_REFINE_F32, "f16": QADC_REFINE_F16, "sq8": QADC_REFINE_SQ8}
_REFINE_DTYPE_NAMES = {v: k for k, v in _REFINE_DTYPES.items()}
QADC_REFINE_L2, QADC_REFINE_IP = 0, 1   # include/qadc.h
_REFINE_METRICS = {"l2": QADC_REFINE_L2, "ip": QADC_REFINE_IP}


def refine_sq_range(vectors, device=0):
    """qadc_refine_sq_range_host: vectors [n][dim] -> (vmin float32 [dim], step float32 [dim]), the range of an SQ8 store
    (DESIGN.md section 11.20): per dimension the minimum of the finite components and (max - min) / 255"""
    v = np.ascontiguousarray(vectors, np.float32)
    if v.ndim != 2 or v.shape[1] < 1:
        raise QadcError("vectors has shape %s, expected [n][dim]" % (v.shape,))
    vmin, step = np.zeros(v.shape[1], np.float32), np.zeros(v.shape[1], np.float32)
    _check(lib().qadc_refine_sq_range_host(_p(v, f32p) if v.shape[0] else None, v.shape[0], v.shape[1], device, _p(vmin, f32p), _p(step, f32p)))
    return vmin, step


def refine_sq_range_device(vectors):
    """the same for a contiguous float32 torch tensor [n][dim] in device memory, read where it lies; the results are numpy arrays"""
    import torch
    if not isinstance(vectors, torch.Tensor) or vectors.ndim != 2 or vectors.dtype != torch.float32 or vectors.device.type != "cuda":
        raise TypeError("vectors must be a 2-d float32 torch.Tensor in device memory")
    if not vectors.is_contiguous():
        raise QadcError("vectors must be contiguous")
    n, dim = int(vectors.shape[0]), int(vectors.shape[1])
    torch.cuda.current_stream(vectors.device).synchronize()
    vmin, step = np.zeros(dim, np.float32), np.zeros(dim, np.float32)
    _check(lib().qadc_refine_sq_range_device(vectors.data_ptr() if n else None, n, dim, vectors.device.index, _p(vmin, f32p), _p(step, f32p)))
    return vmin, step


def refine_keyed_slot(key, bits):
    """qadc_refine_keyed_slot: the home slot of `key` in a keyed store's table of 2**bits slots"""
    return int(lib().qadc_refine_keyed_slot(int(key) & 0xFFFFFFFF, int(bits)))


class Refine:
    """The original vectors in device memory, for exact re-ranking (qadc_refine_*): dense over the keys
    [lo, lo + rows), row r the vector of key lo + r, kept as float32 ("f32") or float16 ("f16").  rerank() reorders candidate keys —
    a search's, with a larger R than wanted — by their exact squared L2 distance; AdcIndex.search_refined, .search_refined_device
    and Index.search_refined compose the two.
    keyed=True (qadc_refine_create_keyed; section 11.14): a map from key to vector in place of the dense range, filled by put(),
    emptied by remove(); add() belongs to the dense kind, put() and remove() to the keyed one (QadcError otherwise).
    dtype="sq8" (qadc_refine_create_sq8; section 11.20): one byte per component under the range vmin=, step= (float32 [dim] each, as
    refine_sq_range gives them); from_vectors() finds the range, creates and adds in one call.
    metric="ip" (qadc_refine_set_metric; section 11.23): rerank, knn, knn_probed and what is composed from them rank by the inner
    product, larger first — `dist` then holds the scores, descending, and -inf behind sizes[q]; the range calls raise.  set_metric()
    changes it at any time; the rows are the same under both."""

    def __init__(self, dim, dtype="f32", device=0, keyed=False, vmin=None, step=None, metric="l2"):
        if dtype not in _REFINE_DTYPES:
            raise ValueError('dtype is "f32", "f16" or "sq8", not %r' % (dtype,))
        if metric not in _REFINE_METRICS:
            raise ValueError('metric is "l2" or "ip", not %r' % (metric,))
        self.dim, self.dtype, self.device, self.keyed = int(dim), dtype, device, bool(keyed)
        self._h = C.c_void_p()
        if dtype == "sq8":
            if vmin is None or step is None:
                raise ValueError('dtype "sq8" needs vmin= and step= (refine_sq_range)')
            vmin, step = np.ascontiguousarray(vmin, np.float32).reshape(-1), np.ascontiguousarray(step, np.float32).reshape(-1)
            if vmin.shape[0] != self.dim or step.shape[0] != self.dim:
                raise ValueError("vmin and step have %d and %d entries for dim %d" % (vmin.shape[0], step.shape[0], self.dim))
            _check(lib().qadc_refine_create_sq8(C.byref(self._h), self.dim, _p(vmin, f32p), _p(step, f32p), int(self.keyed), device))
            self.set_metric(metric)
            return
        if vmin is not None or step is not None:
            raise ValueError('vmin= and step= belong to dtype "sq8"')
        create = lib().qadc_refine_create_keyed if keyed else lib().qadc_refine_create
        _check(create(C.byref(self._h), int(dim), _REFINE_DTYPES[dtype], device))
        self.set_metric(metric)

    def set_metric(self, metric):
        """qadc_refine_set_metric: "l2" or "ip" for every later rerank, knn and knn_probed call; host state only"""
        if metric not in _REFINE_METRICS:
            raise ValueError('metric is "l2" or "ip", not %r' % (metric,))
        _check(lib().qadc_refine_set_metric(self._h, _REFINE_METRICS[metric]))

    @property
    def metric(self):
        """qadc_refine_metric: "l2" or "ip"."""
        m = C.c_int(-1)
        _check(lib().qadc_refine_metric(self._h, C.byref(m)))
        return {v: k for k, v in _REFINE_METRICS.items()}[m.value]

    @classmethod
    def from_vectors(cls, vectors, dtype="f32", device=0, first_key=0, metric="l2"):
        """A dense store holding vectors [n][dim] under the keys first_key ..; an "sq8" store takes the range of these vectors"""
        v = np.ascontiguousarray(vectors, np.float32)
        if v.ndim != 2:
            raise QadcError("vectors has shape %s, expected [n][dim]" % (v.shape,))
        if dtype == "sq8":
            vmin, step = refine_sq_range(v, device)
            self = cls(v.shape[1], "sq8", device, vmin=vmin, step=step, metric=metric)
        else:
            self = cls(v.shape[1], dtype, device, metric=metric)
        if v.shape[0]:
            self.add(v, first_key)
        return self

    def sq_info(self):
        """qadc_refine_sq_info -> dict(vmin float32 [dim], step float32 [dim], clamped: components written outside the range)"""
        vmin, step, clamped = np.zeros(self.dim, np.float32), np.zeros(self.dim, np.float32), C.c_uint64(0)
        _check(lib().qadc_refine_sq_info(self._h, _p(vmin, f32p), _p(step, f32p), C.byref(clamped)))
        return dict(vmin=vmin, step=step, clamped=int(clamped.value))

    def get(self, keys):
        """keys uint32 [n] -> (vectors float32 [n][dim], found bool [n]): the rows as floats, decoded by the store's type; a key the
        store does not hold gives a row of NaN (0x7FC00000) and found False"""
        k = np.ascontiguousarray(np.asarray(keys, np.uint32).reshape(-1))
        out, found = np.zeros((k.shape[0], self.dim), np.float32), np.zeros(k.shape[0], np.uint8)
        _check(lib().qadc_refine_get(self._h, _p(k, u32p), k.shape[0], _p(out, f32p), _p(found, C.POINTER(C.c_uint8))))
        return out, found.astype(bool)

    def get_device(self, keys, out=None):
        """get() for an int32 torch tensor [n] of the store's device that carries the keys' uint32 bits -> (vectors float32 [n][dim],
        found uint8 [n]) on that device.  out: the two tensors to write into."""
        import torch
        if getattr(keys, "ndim", 0) != 1:
            raise TypeError("keys must be a 1-d torch.Tensor")
        n = int(keys.shape[0])
        k = self._tensor(keys, "int32", (n,), "keys")
        dev = torch.device("cuda", self.device)
        if out is None:
            out = (torch.zeros((n, self.dim), dtype=torch.float32, device=dev), torch.zeros((n,), dtype=torch.uint8, device=dev))
        ov = self._tensor(out[0], "float32", (n, self.dim), "out vectors")
        of = self._tensor(out[1], "uint8", (n,), "out found")
        self._sync()
        _check(lib().qadc_refine_get_device(self._h, k.data_ptr(), n, ov.data_ptr(), of.data_ptr()))
        return ov, of

    # ---- the keyed kind ----
    def put(self, vectors, labels):
        """vectors [n][dim], labels uint32 [n]: the vector of key labels[i] becomes vectors[i]; a key not held becomes held, the
        last occurrence of a key wins.  0xFFFFFFFF is refused (rerank's filler key) and the store left as it was."""
        v = np.ascontiguousarray(vectors, np.float32)
        if v.ndim != 2 or v.shape[1] != self.dim:
            raise QadcError("vectors has shape %s, expected [n][%d]" % (v.shape, self.dim))
        lab = np.ascontiguousarray(np.asarray(labels, np.uint32).reshape(-1))
        if lab.shape[0] != v.shape[0]:
            raise ValueError("labels has %d entries for %d vectors" % (lab.shape[0], v.shape[0]))
        _check(lib().qadc_refine_put(self._h, _p(v, f32p), _p(lab, u32p), v.shape[0]))

    def put_device(self, vectors, labels):
        """the same from torch tensors of the store's device, read where they lie: vectors float32 [n][dim], labels int32 [n]
        carrying the uint32 bits"""
        if getattr(vectors, "ndim", 0) != 2:
            raise TypeError("vectors must be a 2-d torch.Tensor")
        n = int(vectors.shape[0])
        t = self._tensor(vectors, "float32", (n, self.dim), "vectors")
        lab = self._tensor(labels, "int32", (n,), "labels")
        self._sync()
        _check(lib().qadc_refine_put_device(self._h, t.data_ptr(), lab.data_ptr(), n))

    def remove(self, labels):
        """every listed key that is held leaves -> how many left (a key listed twice counts once)"""
        lab = np.ascontiguousarray(np.asarray(labels, np.uint32).reshape(-1))
        removed = C.c_uint64(0)
        _check(lib().qadc_refine_remove(self._h, _p(lab, u32p), lab.shape[0], C.byref(removed)))
        return int(removed.value)

    def remove_device(self, labels):
        """remove() for an int32 torch tensor [n] of the store's device that carries the keys' uint32 bits"""
        if getattr(labels, "ndim", 0) != 1:
            raise TypeError("labels must be a 1-d torch.Tensor")
        lab = self._tensor(labels, "int32", (int(labels.shape[0]),), "labels")
        self._sync()
        removed = C.c_uint64(0)
        _check(lib().qadc_refine_remove_device(self._h, lab.data_ptr(), int(lab.shape[0]), C.byref(removed)))
        return int(removed.value)

    def keyed_info(self):
        """-> dict(live, rows_allocated, rows_free, table_slots, table_used, bytes) of a keyed store"""
        out = [C.c_uint64(0) for _ in range(6)]
        _check(lib().qadc_refine_keyed_info(self._h, *[C.byref(x) for x in out]))
        return dict(zip(("live", "rows_allocated", "rows_free", "table_slots", "table_used", "bytes"), (int(x.value) for x in out)))

    @classmethod
    def create_raw(cls, dim, dtype, device=0):
        """The C call as it is (dtype: an int)."""
        self = cls.__new__(cls)
        self.dim, self.dtype, self.device = dim, dtype, device
        self._h = C.c_void_p()
        _check(lib().qadc_refine_create(C.byref(self._h), dim, dtype, device))
        return self

    def close(self):
        if getattr(self, "_h", None):
            lib().qadc_refine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _first_key(self, first_key):
        if first_key is not None:
            return int(first_key)
        i = self.info()
        return i["lo"] + i["rows"]                                         # continue; 0 on an empty store

    def add(self, vectors, first_key=None):
        """vectors [n][dim] become the rows of the keys first_key .. first_key + n - 1; None continues the store (0 on an empty one)"""
        v = np.ascontiguousarray(vectors, np.float32)
        if v.ndim != 2 or v.shape[1] != self.dim:
            raise QadcError("vectors has shape %s, expected [n][%d]" % (v.shape, self.dim))
        _check(lib().qadc_refine_add(self._h, _p(v, f32p), v.shape[0], self._first_key(first_key)))

    def add_raw(self, vectors, count, first_key):
        """The C call as it is (vectors: a float32 array or None)."""
        _check(lib().qadc_refine_add(self._h, _p(vectors, f32p), count, first_key))

    def add_device(self, vectors, first_key=None):
        """the same from a contiguous float32 torch tensor [n][dim] on the store's device, read where it lies"""
        if getattr(vectors, "ndim", 0) != 2:
            raise TypeError("vectors must be a 2-d torch.Tensor")
        t = self._tensor(vectors, "float32", (int(vectors.shape[0]), self.dim), "vectors")
        self._sync()
        _check(lib().qadc_refine_add_device(self._h, t.data_ptr(), int(t.shape[0]), self._first_key(first_key)))

    def reserve(self, rows):
        """room for `rows` rows in all: the adds up to there relocate nothing"""
        _check(lib().qadc_refine_reserve(self._h, int(rows)))

    def info(self):
        """-> dict(dim, dtype "f32" | "f16" | "sq8", lo, rows, bytes: the allocation's)"""
        dim, dtype, lo, rows, nbytes = C.c_int(0), C.c_int(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().qadc_refine_info(self._h, C.byref(dim), C.byref(dtype), C.byref(lo), C.byref(rows), C.byref(nbytes)))
        return dict(dim=dim.value, dtype=_REFINE_DTYPE_NAMES[dtype.value], lo=int(lo.value), rows=int(rows.value),
                    bytes=int(nbytes.value))

    def relocations(self):
        """adds that moved the rows held to grow the allocation"""
        return int(lib().qadc_refine_relocations(self._h))

    def rerank(self, queries, keys, R, counts=None, values=None):
        """queries [nq][dim], keys uint32 [nq][r_in], counts int32 [nq] or None, values float32 [nq][r_in] or None (FLT_MAX marks an
        entry that is no candidate) -> (keys uint32 [nq][R], dist float32 [nq][R], sizes int32 [nq], missing): per query the first R
        of its candidates by (exact squared L2 distance, key), every key once; behind sizes[q]: key 0xFFFFFFFF, distance +inf;
        missing = the candidates whose key the store does not hold."""
        q = np.ascontiguousarray(queries, np.float32)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise QadcError("queries has shape %s, expected [nq][%d]" % (q.shape, self.dim))
        nq = q.shape[0]
        k = np.ascontiguousarray(keys, np.uint32).reshape(nq, -1)
        c = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(nq)
        v = None if values is None else np.ascontiguousarray(values, np.float32).reshape(k.shape)
        return self.rerank_raw(nq, q, k.shape[1], k, c, v, int(R))

    def rerank_raw(self, nq, queries, r_in, keys, counts, values, R, outputs=True):
        """The C call as it is (arrays of the right dtype, or None)."""
        ok = np.zeros((max(nq, 0), max(R, 0)), np.uint32) if outputs else None
        od = np.zeros((max(nq, 0), max(R, 0)), np.float32) if outputs else None
        osz = np.zeros(max(nq, 0), np.int32) if outputs else None
        missing = C.c_uint64(0)
        _check(lib().qadc_refine_rerank(self._h, nq, _p(queries, f32p), r_in, _p(keys, u32p), _p(counts, i32p), _p(values, f32p), R,
                                        _p(ok, u32p), _p(od, f32p), _p(osz, i32p), C.byref(missing)))
        return ok, od, osz, int(missing.value)

    # ---- device memory in, device memory out: torch tensors by data_ptr() (torch is imported here only) ----
    def _tensor(self, t, dtype, shape, what):
        import torch
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor, not %s" % (what, type(t).__name__))
        if t.dtype != getattr(torch, dtype):
            raise TypeError("%s must be %s, not %s" % (what, dtype, t.dtype))
        if t.device.type != "cuda" or t.device.index != self.device:
            raise QadcError("%s is on %s; the store is on device %d" % (what, t.device, self.device))
        if not t.is_contiguous():
            raise QadcError("%s must be contiguous" % what)
        if tuple(t.shape) != tuple(shape):
            raise QadcError("%s has shape %s, expected %s" % (what, tuple(t.shape), tuple(shape)))
        return t

    def _sync(self):
        import torch
        torch.cuda.current_stream(torch.device("cuda", self.device)).synchronize()   # inputs are complete before the call

    def rerank_device(self, queries, keys, R, counts=None, values=None):
        """rerank() on torch tensors of the store's device: queries float32 [nq][dim], keys int32 [nq][r_in] carrying the uint32 bits
        (as search_device returns them), counts int32 [nq] or None (clamped to [0, r_in]), values float32 [nq][r_in] or None ->
        (keys int32 [nq][R], dist float32 [nq][R], sizes int32 [nq]) on that device, and missing (an int)."""
        import torch
        if getattr(queries, "ndim", 0) != 2 or getattr(keys, "ndim", 0) != 2:
            raise TypeError("queries and keys must be 2-d torch.Tensors")
        nq, r_in, R = int(queries.shape[0]), int(keys.shape[1]), int(R)
        q = self._tensor(queries, "float32", (nq, self.dim), "queries")
        k = self._tensor(keys, "int32", (nq, r_in), "keys")
        c = None if counts is None else self._tensor(counts, "int32", (nq,), "counts")
        v = None if values is None else self._tensor(values, "float32", (nq, r_in), "values")
        dev = torch.device("cuda", self.device)
        ok = torch.zeros((nq, max(R, 0)), dtype=torch.int32, device=dev)
        od = torch.zeros((nq, max(R, 0)), dtype=torch.float32, device=dev)
        osz = torch.zeros((nq,), dtype=torch.int32, device=dev)
        self._sync()
        missing = C.c_uint64(0)
        _check(lib().qadc_refine_rerank_device(self._h, nq, q.data_ptr(), r_in, k.data_ptr(), None if c is None else c.data_ptr(),
                                               None if v is None else v.data_ptr(), R, ok.data_ptr(), od.data_ptr(), osz.data_ptr(),
                                               C.byref(missing)))
        return ok, od, osz, int(missing.value)

    # ---- exhaustive search (qadc_refine_knn) ----
    def knn(self, queries, R, filter=None):
        """queries [nq][dim] -> (keys uint32 [nq][R], dist float32 [nq][R], sizes int32 [nq]): per query the first R of EVERY key the
        store holds that passes `filter` (an AdcFilter of the store's device, or None), by (exact squared L2 distance, key) — rerank()
        fed every held key, bit for bit; behind sizes[q]: key 0xFFFFFFFF, distance +inf.  1 <= R <= 1024."""
        q = np.ascontiguousarray(queries, np.float32)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise QadcError("queries has shape %s, expected [nq][%d]" % (q.shape, self.dim))
        return self.knn_raw(q.shape[0], q, int(R), filter)

    def knn_raw(self, nq, queries, R, filter=None, outputs=True):
        """The C call as it is (queries: a float32 array or None; filter: an AdcFilter or None)."""
        ok = np.zeros((max(nq, 0), max(R, 0)), np.uint32) if outputs else None
        od = np.zeros((max(nq, 0), max(R, 0)), np.float32) if outputs else None
        osz = np.zeros(max(nq, 0), np.int32) if outputs else None
        _check(lib().qadc_refine_knn(self._h, nq, _p(queries, f32p), R, None if filter is None else filter._h, _p(ok, u32p), _p(od, f32p),
                                     _p(osz, i32p)))
        return ok, od, osz

    def knn_device(self, queries, R, filter=None, out=None):
        """knn() on torch tensors of the store's device: queries float32 [nq][dim] -> (keys int32 [nq][R] carrying the uint32 bits,
        dist float32 [nq][R], sizes int32 [nq]) on that device; nothing crosses the bus.  out: the three tensors to write into."""
        import torch
        if getattr(queries, "ndim", 0) != 2:
            raise TypeError("queries must be a 2-d torch.Tensor")
        nq, R = int(queries.shape[0]), int(R)
        q = self._tensor(queries, "float32", (nq, self.dim), "queries")
        dev = torch.device("cuda", self.device)
        if out is None:
            out = (torch.zeros((nq, max(R, 0)), dtype=torch.int32, device=dev), torch.zeros((nq, max(R, 0)), dtype=torch.float32, device=dev),
                   torch.zeros((nq,), dtype=torch.int32, device=dev))
        ok = self._tensor(out[0], "int32", (nq, max(R, 0)), "out keys")
        od = self._tensor(out[1], "float32", (nq, max(R, 0)), "out dist")
        osz = self._tensor(out[2], "int32", (nq,), "out sizes")
        self._sync()
        _check(lib().qadc_refine_knn_device(self._h, nq, q.data_ptr(), R, None if filter is None else filter._h, ok.data_ptr(), od.data_ptr(),
                                            osz.data_ptr()))
        return ok, od, osz

    # ---- probed exact search (qadc_refine_knn_probed) ----
    def knn_probed(self, index, queries, assign, R, filter=None):
        """index: an AdcIndex (owned, or a view of a 4-bit index) of the store's device; queries [nq][dim], assign int32 [nq][ma] ->
        (keys uint32 [nq][R], dist float32 [nq][R], sizes int32 [nq], missing): per query the first R, by (exact squared L2 distance,
        key), of the keys of every row of the partitions its list probes — rerank() fed those keys with no limit on their number,
        bit for bit.  A key must pass the index's set_filter and `filter`; a key the store does not hold is missing, per entry; a key
        reached through several rows is kept once.  An entry of assign outside [0, partitions) raises."""
        q = np.ascontiguousarray(queries, np.float32)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise QadcError("queries has shape %s, expected [nq][%d]" % (q.shape, self.dim))
        a = np.ascontiguousarray(assign, np.int32)
        if a.ndim == 1:
            a = a.reshape(q.shape[0], -1)
        if a.ndim != 2 or a.shape[0] != q.shape[0]:
            raise QadcError("assign has shape %s, expected [%d][ma]" % (a.shape, q.shape[0]))
        return self.knn_probed_raw(index, q.shape[0], q, a.shape[1], a, int(R), filter)

    def knn_probed_raw(self, index, nq, queries, ma, assign, R, filter=None, outputs=True):
        """The C call as it is (index: an AdcIndex or None; queries, assign: arrays or None; filter: an AdcFilter or None)."""
        ok = np.zeros((max(nq, 0), max(R, 0)), np.uint32) if outputs else None
        od = np.zeros((max(nq, 0), max(R, 0)), np.float32) if outputs else None
        osz = np.zeros(max(nq, 0), np.int32) if outputs else None
        missing = C.c_uint64(0)
        _check(lib().qadc_refine_knn_probed(self._h, None if index is None else index._h, nq, _p(queries, f32p), ma, _p(assign, i32p), R,
                                            None if filter is None else filter._h, _p(ok, u32p), _p(od, f32p), _p(osz, i32p), C.byref(missing)))
        return ok, od, osz, int(missing.value)

    def knn_probed_device(self, index, queries, assign, R, filter=None, out=None):
        """knn_probed() on torch tensors of the store's device: queries float32 [nq][dim], assign int32 [nq][ma] -> (keys int32 [nq][R]
        carrying the uint32 bits, dist float32 [nq][R], sizes int32 [nq]) on that device, and missing (an int).  An entry of assign
        outside [0, partitions) is skipped.  The probe numbers are read back by the planner; nothing else of the arrays crosses the
        bus.  out: the three tensors to write into."""
        import torch
        if getattr(queries, "ndim", 0) != 2 or getattr(assign, "ndim", 0) != 2:
            raise TypeError("queries and assign must be 2-d torch.Tensors")
        nq, ma, R = int(queries.shape[0]), int(assign.shape[1]), int(R)
        q = self._tensor(queries, "float32", (nq, self.dim), "queries")
        a = self._tensor(assign, "int32", (nq, ma), "assign")
        dev = torch.device("cuda", self.device)
        if out is None:
            out = (torch.zeros((nq, max(R, 0)), dtype=torch.int32, device=dev), torch.zeros((nq, max(R, 0)), dtype=torch.float32, device=dev),
                   torch.zeros((nq,), dtype=torch.int32, device=dev))
        ok = self._tensor(out[0], "int32", (nq, max(R, 0)), "out keys")
        od = self._tensor(out[1], "float32", (nq, max(R, 0)), "out dist")
        osz = self._tensor(out[2], "int32", (nq,), "out sizes")
        self._sync()
        missing = C.c_uint64(0)
        _check(lib().qadc_refine_knn_probed_device(self._h, index._h, nq, q.data_ptr(), ma, a.data_ptr(), R, None if filter is None else filter._h,
                                                   ok.data_ptr(), od.data_ptr(), osz.data_ptr(), C.byref(missing)))
        return ok, od, osz, int(missing.value)

    def set_knn_plan(self, chunk_rows=0, pass_nq=0):
        """qadc_refine_set_knn_plan: the rows of a group per launch and the queries per pass of the later knn calls (0: the plan's
        default) — a tuning and test knob; no value changes a result"""
        _check(lib().qadc_refine_set_knn_plan(self._h, int(chunk_rows), int(pass_nq)))

    # ---- exact range search (qadc_refine_range*, qadc_refine_rerank_range*) ----
    def _queries(self, queries):
        q = np.ascontiguousarray(queries, np.float32)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise QadcError("queries has shape %s, expected [nq][%d]" % (q.shape, self.dim))
        return q

    def range_collect_raw(self, capacity):
        """The C call as it is: -> (rc, keys [capacity], dist [capacity])"""
        keys = np.zeros(max(capacity, 1), np.uint32)
        dist = np.zeros(max(capacity, 1), np.float32)
        return lib().qadc_refine_range_collect(self._h, capacity, _p(keys, u32p), _p(dist, f32p)), keys, dist

    def range_collect(self, lims=None):
        """qadc_refine_range_collect: (keys uint32, dist float32) of the range result the store holds, any number of times; lims: the
        array the range call returned (default: the last one made through this object)."""
        n = int(lims[-1]) if lims is not None else getattr(self, "_range_rows", 0)
        rc, keys, dist = self.range_collect_raw(n)
        _check(rc)
        return keys[:n], dist[:n]

    def _range_collect_device(self, lims):
        import torch
        dev = torch.device("cuda", self.device)
        n = int(lims[-1])
        keys = torch.zeros((n,), dtype=torch.int32, device=dev)          # the uint32 keys' bits
        dist = torch.zeros((n,), dtype=torch.float32, device=dev)
        self._sync()                                                     # the zero fills are complete before the call
        _check(lib().qadc_refine_range_collect_device(self._h, n, keys.data_ptr(), dist.data_ptr()))
        return keys, dist

    def range(self, queries, radius, filter=None):
        """queries [nq][dim], radius a scalar or [nq] -> (lims int64 [nq+1], keys uint32, dist float32): for query q, rows
        [lims[q], lims[q+1]) = EVERY key the store holds that passes `filter` (an AdcFilter of the store's device, or None) and whose exact
        squared L2 distance is < radius[q] (a float compare: NaN keeps nothing), ascending by (distance, key); refine::range."""
        q = self._queries(queries)
        nq = q.shape[0]
        r = AdcIndex._radius(radius, nq)
        lims = np.zeros(nq + 1, np.uint64)
        _check(lib().qadc_refine_range(self._h, nq, _p(q, f32p), _p(r, f32p), None if filter is None else filter._h, _p(lims, u64p)))
        self._range_rows = int(lims[-1])
        keys, dist = self.range_collect(lims)
        return lims.astype(np.int64), keys, dist

    def range_device(self, queries, radius, filter=None):
        """range() for a float32 torch tensor [nq][dim] of the store's device -> (lims int64 numpy, keys int32 tensor carrying the
        uint32 bits, dist float32 tensor): only radius and lims cross the bus."""
        if getattr(queries, "ndim", 0) != 2:
            raise TypeError("queries must be a 2-d torch.Tensor")
        nq = int(queries.shape[0])
        q = self._tensor(queries, "float32", (nq, self.dim), "queries")
        r = AdcIndex._radius(radius, nq)
        lims = np.zeros(nq + 1, np.uint64)
        self._sync()
        _check(lib().qadc_refine_range_device(self._h, nq, q.data_ptr(), _p(r, f32p), None if filter is None else filter._h, _p(lims, u64p)))
        self._range_rows = int(lims[-1])
        keys, dist = self._range_collect_device(lims)
        return lims.astype(np.int64), keys, dist

    @staticmethod
    def _in_lims(lims, nq):
        a = np.asarray(lims)
        if a.shape != (nq + 1,) or (a.dtype.kind == "i" and (a < 0).any()):
            raise ValueError("lims has one entry per query and one more (%d), none negative, not shape %s" % (nq + 1, a.shape))
        return np.ascontiguousarray(a, np.uint64)

    def rerank_range(self, queries, lims, keys, radius):
        """queries [nq][dim], lims [nq+1] and keys uint32 [lims[nq]] (a range result in CSR form), radius a scalar or [nq] ->
        (lims int64 [nq+1], keys uint32, dist float32, missing): per query those of its candidates the store holds whose exact squared
        L2 distance is < radius[q], ascending by (distance, key), every key once; missing = the candidates whose key the store does not
        hold.  No limit on the candidates of a query; refine::rerank_range."""
        q = self._queries(queries)
        nq = q.shape[0]
        il = self._in_lims(lims, nq)
        k = np.ascontiguousarray(np.asarray(keys, np.uint32).reshape(-1))
        if k.shape[0] < int(il[-1]):
            raise ValueError("keys has %d entries, lims[nq] is %d" % (k.shape[0], int(il[-1])))
        r = AdcIndex._radius(radius, nq)
        out = np.zeros(nq + 1, np.uint64)
        missing = C.c_uint64(0)
        _check(lib().qadc_refine_rerank_range(self._h, nq, _p(q, f32p), _p(il, u64p), _p(k, u32p) if k.shape[0] else None, _p(r, f32p),
                                              _p(out, u64p), C.byref(missing)))
        self._range_rows = int(out[-1])
        okeys, dist = self.range_collect(out)
        return out.astype(np.int64), okeys, dist, int(missing.value)

    def rerank_range_device(self, queries, lims, keys, radius):
        """rerank_range() on torch tensors of the store's device: queries float32 [nq][dim], keys int32 [n >= lims[nq]] carrying the
        uint32 bits (as AdcIndex.range_search_device returns them); lims stays a host array -> (lims int64 numpy, keys int32 tensor,
        dist float32 tensor, missing)."""
        if getattr(queries, "ndim", 0) != 2 or getattr(keys, "ndim", 0) != 1:
            raise TypeError("queries must be a 2-d and keys a 1-d torch.Tensor")
        nq = int(queries.shape[0])
        q = self._tensor(queries, "float32", (nq, self.dim), "queries")
        k = self._tensor(keys, "int32", (int(keys.shape[0]),), "keys")
        il = self._in_lims(lims, nq)
        if int(k.shape[0]) < int(il[-1]):
            raise ValueError("keys has %d entries, lims[nq] is %d" % (int(k.shape[0]), int(il[-1])))
        r = AdcIndex._radius(radius, nq)
        out = np.zeros(nq + 1, np.uint64)
        missing = C.c_uint64(0)
        self._sync()
        _check(lib().qadc_refine_rerank_range_device(self._h, nq, q.data_ptr(), _p(il, u64p), k.data_ptr() if k.shape[0] else None, _p(r, f32p),
                                                     _p(out, u64p), C.byref(missing)))
        self._range_rows = int(out[-1])
        okeys, dist = self._range_collect_device(out)
        return out.astype(np.int64), okeys, dist, int(missing.value)

    def set_range_plan(self, region_rows=0, chunk_rows=0, pass_nq=0):
        """qadc_refine_set_range_plan: the words of a query's region in the first run, the rows of a group per launch and the queries
        per pass of the later range calls (0: the plan's default) — a tuning and test knob; no value changes a result"""
        _check(lib().qadc_refine_set_range_plan(self._h, int(region_rows), int(chunk_rows), int(pass_nq)))

    def range_reruns(self):
        """passes of range() that ran a second time because a query's region overflowed"""
        return int(lib().qadc_refine_range_reruns(self._h))
