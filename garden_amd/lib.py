"""ctypes binding of libgarden_vis.so (C-ABI: include/garden_vis.h).

Plumbing for tests and bench.py. Loading fails loudly when the HIP library is missing; creating a
context fails loudly (GvError) when there is no gfx950 device — there is no CPU fallback anywhere in
this package.
"""
import ctypes as C
import os

import numpy as np

from .pools import GV_NONE, mesh_layout_offsets, transform_layout_offsets

_HERE = os.path.dirname(os.path.abspath(__file__))
# GV_LIB_PATH: dev A/Bs against another build of the same library (e.g. a previous round's kernels); never a fallback
LIB_PATH = os.environ.get("GV_LIB_PATH") or os.path.join(_HERE, "lib", "libgarden_vis.so")

GV_MAX_POOLS, GV_MAX_VIEWS, GV_MAX_MIPS, GV_K_COUNT = 16, 8, 16, 6
GV_MAX_PYRAMIDS = 8  # pyramid slots of a context (hiz_select)
GV_OK, GV_E_ARG, GV_E_HIP, GV_E_OOM, GV_E_RCCL, GV_E_STATE, GV_E_NODEVICE, GV_E_TIMEOUT = 0, -1, -2, -3, -4, -5, -6, -7
GV_HIZ_RULE_REFERENCE, GV_HIZ_RULE_CONSERVATIVE = 0, 1
GV_CONFIG_PROFILE_EVENTS = 1
GV_CONFIG_PROFILE_CULL_ONLY = 2
GV_CONFIG_KEEP_SLOT_ORDER = 4
GV_CONFIG_BLOCK_BOUNDS = 8
GV_CONFIG_HIZ_RG16F = 16
GV_CONFIG_LINEAR_SCAN = 32
GV_DIRTY_TRANSFORM, GV_DIRTY_HIERARCHY, GV_DIRTY_MESH, GV_DIRTY_PAYLOAD, GV_DIRTY_GEOMETRY, GV_DIRTY_LOD = 0, 1, 2, 3, 4, 5
GV_DIRTY_OCCLUDER = 6
GV_MAX_DRAW_INSTANCES = 65535
GV_MAX_GEOMETRIES = 65536
GV_COMMANDS_MERGE_RUNS = 1
GV_GROUP_BY_LOD = 1
GV_SWEEP_VALU, GV_SWEEP_MFMA, GV_SWEEP_WITH_CULL, GV_SWEEP_WITH_CULL_VALU, GV_SWEEP_INCREMENTAL = 0, 1, 2, 3, 4
GV_MEM_HOST, GV_MEM_DEVICE = 0, 1
GV_EXCHANGE_ALLGATHER, GV_EXCHANGE_P2P, GV_EXCHANGE_BROADCAST, GV_EXCHANGE_PEER = 0, 1, 2, 3
KERNEL_NAMES = ["cull", "scan", "emit", "hiz", "sweep", "sort"]


class GvConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("hiz_rule", C.c_uint32), ("flags", C.c_uint32)]


class GvTransformLayout(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("entity", "parent", "position", "scale", "rotation", "self_active",
                                          "ancestors_active", "model_with_ancestors")]


class GvMeshLayout(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("entity", "is_enabled", "is_visible", "aabb_min", "aabb_max")]


class GvView(C.Structure):
    _fields_ = [("view_proj", C.c_float * 16), ("camera_position", C.c_float * 4), ("camera_offset", C.c_float * 4),
                ("shadow_pass", C.c_int8), ("use_hiz", C.c_uint8), ("distance_2d", C.c_uint8),
                ("emit_records", C.c_uint8)]


class GvResult(C.Structure):
    _fields_ = [("visible_idx", C.POINTER(C.c_uint32)), ("baked_model", C.POINTER(C.c_float)),
                ("distance_sq", C.POINTER(C.c_float)), ("is_visible", C.POINTER(C.c_uint8)),
                ("draw_count", C.c_uint32), ("instance_count", C.c_uint32)]


class GvRecordLayout(C.Structure):
    _fields_ = [("stride", C.c_uint32), ("component_offset", C.c_uint32), ("baked_model", C.c_uint32), ("distance_sq", C.c_uint32),
                ("buffer_index", C.c_uint32), ("component_stride", C.c_uint32), ("buffer_index_value", C.c_uint32)]


class GvDeviceResult(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("visible_idx", "baked_model", "distance_sq", "is_visible", "draw_count")]


class GvStats(C.Structure):
    _fields_ = [("launches", C.c_uint64 * GV_K_COUNT), ("device_ms", C.c_double * GV_K_COUNT),
                ("upload_bytes", C.c_uint64), ("max_depth", C.c_uint32), ("transform_count", C.c_uint32),
                ("mesh_count", C.c_uint32 * GV_MAX_POOLS), ("bounds_blocks_total", C.c_uint64),
                ("bounds_blocks_examined", C.c_uint64), ("mirror_reorders", C.c_uint64), ("record_targets_lost", C.c_uint64),
                ("exchanges", C.c_uint64), ("exchange_tail_rounds", C.c_uint64)]


GV_EXCHANGE_MAX_RANKS = 64


class GvExchangeFrame(C.Structure):
    _fields_ = [("gathered_device", C.c_void_p), ("row_words", C.c_uint32), ("world_size", C.c_uint32), ("frame", C.c_uint64),
                ("room", C.c_uint32 * GV_EXCHANGE_MAX_RANKS), ("travelled_words", C.c_uint32 * GV_EXCHANGE_MAX_RANKS),
                ("counts", C.c_uint32 * GV_EXCHANGE_MAX_RANKS), ("tail_words", C.c_uint32 * GV_EXCHANGE_MAX_RANKS), ("cut_ranks", C.c_uint64),
                ("complete", C.c_uint32), ("mode", C.c_uint32), ("ready_event", C.c_void_p),
                ("items", C.c_uint32), ("item_counts", C.POINTER(C.c_uint32))]


GV_EXCHANGE_MAX_ITEMS = 128
GV_RESULTS_MAP_RECORDS, GV_RESULTS_MAP_VISIBLE = 1, 2


class GvExchangeItem(C.Structure):
    _fields_ = [("pool_id", C.c_uint32), ("view_index", C.c_uint32), ("index_base", C.c_uint32)]


class GvPickRay(C.Structure):
    _fields_ = [("origin", C.c_float * 4), ("direction", C.c_float * 4)]


class GvPickHit(C.Structure):
    _fields_ = [("pool_id", C.c_uint32), ("slot", C.c_uint32), ("distance_sq", C.c_float), ("reserved", C.c_uint32)]


GV_MAX_PICK_RAYS = 8


class GvInstanceLayout(C.Structure):
    _fields_ = [("stride", C.c_uint32), ("mvp", C.c_uint32), ("model", C.c_uint32), ("slot", C.c_uint32), ("distance_sq", C.c_uint32)]


class GvGeometry(C.Structure):
    _fields_ = [("count", C.c_uint32), ("first", C.c_uint32), ("vertex_offset", C.c_int32)]


GEOMETRY_DTYPE = np.dtype([("count", np.uint32), ("first", np.uint32), ("vertex_offset", np.int32)])


GV_MAX_CLUSTERS = 1 << 22
GV_MAX_GEOMETRY_CLUSTERS = 65535
GV_CLUSTERS_FRUSTUM_ONLY = 1
GV_CLUSTER_RUN_SPAN = 256
GV_CLUSTERS_RUNS = 2  # gv_pool_cull_cluster_cones and gv_pool_cull_cluster_lods only


class GvCluster(C.Structure):
    _fields_ = [("box_min", C.c_float * 3), ("first", C.c_uint32), ("box_max", C.c_float * 3), ("count", C.c_uint32)]


class GvClusterRange(C.Structure):
    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32)]


CLUSTER_DTYPE = np.dtype([("box_min", np.float32, (3,)), ("first", np.uint32), ("box_max", np.float32, (3,)), ("count", np.uint32)])
CLUSTER_RANGE_DTYPE = np.dtype([("first", np.uint32), ("count", np.uint32)])
# GvClusterCone: meshopt_Bounds' cone_apex / cone_axis / cone_cutoff as they are; `reserved` is not read
CLUSTER_CONE_DTYPE = np.dtype([("apex", np.float32, (3,)), ("cutoff", np.float32), ("axis", np.float32, (3,)), ("reserved", np.uint32)])
# GvClusterLod: the bounds and error of the group a cluster was simplified from (self) and merged into (parent); `reserved` is not read
CLUSTER_LOD_DTYPE = np.dtype([("self_center", np.float32, (3,)), ("self_radius", np.float32), ("parent_center", np.float32, (3,)),
                              ("parent_radius", np.float32), ("self_error", np.float32), ("parent_error", np.float32), ("reserved", np.uint32, (2,))])
# GvClusterLodView: one per view of the emission; scale 0 switches the LOD test off for the view
CLUSTER_LOD_VIEW_DTYPE = np.dtype([("eye", np.float32, (4,)), ("scale", np.float32), ("near_distance", np.float32), ("reserved", np.float32, (2,))])


GV_MAX_LOD_LEVELS = 8


class GvLodGeometry(C.Structure):
    _fields_ = [("levels", C.c_uint32), ("switch_at", C.c_float * (GV_MAX_LOD_LEVELS - 1))]


LOD_DTYPE = np.dtype([("levels", np.uint32), ("switch_at", np.float32, (GV_MAX_LOD_LEVELS - 1,))])


GV_MAX_BOUNDS_ITEMS = 8


class GvViewBounds(C.Structure):
    _fields_ = [("lo", C.c_float * 3), ("draw_count", C.c_uint32), ("hi", C.c_float * 3), ("nan_records", C.c_uint32)]


BOUNDS_DTYPE = np.dtype([("lo", np.float32, (3,)), ("draw_count", np.uint32), ("hi", np.float32, (3,)), ("nan_records", np.uint32)])


class GvOccluderCounts(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("drawn", "no_box", "behind", "range", "flat", "small")]


OCCLUDER_COUNT_NAMES = tuple(name for name, _ in GvOccluderCounts._fields_)


class GvReceiverCounts(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("drawn", "flat", "behind", "range", "outside", "reserved")]


RECEIVER_COUNT_NAMES = tuple(name for name, _ in GvReceiverCounts._fields_)


GV_MAX_DELTA_CHANNELS = 4
GV_DELTA_RESTART = 1


class GvViewDelta(C.Structure):
    _fields_ = [("appeared", C.POINTER(C.c_uint32)), ("vanished", C.POINTER(C.c_uint32)), ("appeared_count", C.c_uint32),
                ("vanished_count", C.c_uint32), ("visible_count", C.c_uint32), ("slots", C.c_uint32)]


GV_KEEP_ADD = 1
GV_PREVIOUS_CUT = 1


class GvPreviousLayout(C.Structure):
    _fields_ = [("stride", C.c_uint32), ("prev_mvp", C.c_uint32), ("has_history", C.c_uint32)]


class GvCommandLayout(C.Structure):
    _fields_ = [("stride", C.c_uint32), ("count", C.c_uint32), ("instance_count", C.c_uint32), ("first", C.c_uint32),
                ("first_instance", C.c_uint32), ("vertex_offset", C.c_uint32), ("draw", C.c_uint32)]


GV_MAX_MERGE_GROUPS = 12
GV_MAX_MERGE_ITEMS = 16


class GvMergeItem(C.Structure):
    _fields_ = [("pool_id", C.c_uint32), ("view_index", C.c_uint32), ("buffer_index", C.c_uint32), ("component_stride", C.c_uint32)]


class GvMergeGroup(C.Structure):
    _fields_ = [("group_id", C.c_uint32), ("item_count", C.c_uint32), ("items", C.POINTER(GvMergeItem)), ("descending", C.c_uint32),
                ("stride", C.c_uint32), ("component_offset", C.c_uint32), ("baked_model", C.c_uint32), ("distance_sq", C.c_uint32),
                ("buffer_index", C.c_uint32), ("dst_device", C.c_void_p), ("capacity_bytes", C.c_size_t)]


class GvColumn(C.Structure):
    _fields_ = [("data", C.c_void_p), ("stride", C.c_uint32)]


GV_MAX_PAYLOAD_FIELDS = 4
GV_MAX_PAYLOAD_BYTES = 64


class GvPayloadField(C.Structure):
    _fields_ = [("data", C.c_void_p), ("stride", C.c_uint32), ("bytes", C.c_uint32)]


class GvTransformColumns(C.Structure):
    _fields_ = [(n, GvColumn) for n in ("entity", "parent", "position", "scale", "rotation", "self_active",
                                        "ancestors_active", "model_with_ancestors")]


class GvMeshColumns(C.Structure):
    _fields_ = [("entity", GvColumn), ("is_enabled", GvColumn), ("aabb_min", GvColumn), ("aabb_max", GvColumn),
                ("is_visible", C.c_void_p), ("is_visible_stride", C.c_uint32)]


class GvScenePool(C.Structure):
    _fields_ = [("component_type", C.c_char_p), ("pool_id", C.c_uint32)]


class GvSceneInfo(C.Structure):
    _fields_ = [("entity_count", C.c_uint32), ("transform_count", C.c_uint32), ("mesh_count", C.c_uint32 * GV_MAX_POOLS),
                ("skipped_entities", C.c_uint32), ("other_components", C.c_uint32), ("duplicate_uids", C.c_uint32),
                ("self_parents", C.c_uint32), ("unresolved_parents", C.c_uint32)]


class GvError(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"libgarden_vis error {code}: {text}")
        self.code = code


# every symbol include/garden_vis.h declares; tests/test_abi.py checks the .so exports all of them
EXPORTS = [
    "gv_abi_version", "gv_create", "gv_destroy", "gv_last_error", "gv_transform_bind", "gv_pool_bind",
    "gv_transform_bind_columns", "gv_pool_bind_columns", "gv_pool_bind_ready",
    "gv_mark_dirty", "gv_hierarchy_rebuild", "gv_sync", "gv_cull", "gv_wait", "gv_results_fetch",
    "gv_result_count", "gv_results_device", "gv_results_copy_idx_device", "gv_results_copy_shard_device", "gv_results_copy_mask_device", "gv_pool_mirror_slots", "gv_pool_mirror_epoch", "gv_sort", "gv_sweep", "gv_get_world",
    "gv_hiz_build", "gv_hiz_rebuild", "gv_hiz_read_level", "gv_hiz_mip_count", "gv_hiz_select", "gv_hiz_drop", "gv_stats", "gv_stats_reset",
    "gv_stream", "gv_debug_stream_peak",
    "gv_scene_parse_json", "gv_scene_parse_bson", "gv_scene_destroy", "gv_scene_info", "gv_scene_transform_columns", "gv_scene_mesh_columns",
    "gv_scene_bind", "gv_scene_extract_tile", "gv_scene_extract_rank", "gv_cell_owner", "gv_scene_tile_maps",
    "gv_exchange_unique_id", "gv_exchange_init", "gv_exchange_init_all", "gv_exchange_init_peers", "gv_exchange_shards", "gv_exchange_visible", "gv_exchange_visible_all", "gv_pool_exchange_visible", "gv_pool_exchange_visible_all", "gv_exchange_acquire", "gv_exchange_acquire_all", "gv_exchange_set_timeout", "gv_exchange_masks", "gv_exchange_shutdown", "gv_exchange_set_mode", "gv_pool_set_index_map",
    "gv_exchange_views", "gv_exchange_views_all", "gv_pool_update_index_map", "gv_pool_set_result_mapping", "gv_host_parallel_ranges", "gv_host_parallel_tasks",
    "gv_pool_results_fetch", "gv_pool_result_count", "gv_pool_results_device", "gv_pool_sort",
    "gv_cull_batch_begin", "gv_cull_batch_end", "gv_pool_set_record_layout", "gv_pool_results_records", "gv_pool_set_record_target",
    "gv_pool_results_instance_bases", "gv_profile_sampling", "gv_profile_samples", "gv_profile_kernels", "gv_pick",
    "gv_pool_set_instance_layout", "gv_pool_emit_instances", "gv_pool_instances_device", "gv_pool_instances_info", "gv_pool_instances_fetch",
    "gv_pool_bind_payload", "gv_pool_set_payload_layout",
    "gv_pool_emit_draw_instances", "gv_pool_set_instance_index_field", "gv_pool_draw_bases_device", "gv_pool_draw_bases_fetch",
    "gv_merge_sorted", "gv_merge_device", "gv_merge_fetch",
    "gv_pool_bind_geometry", "gv_pool_set_command_layout", "gv_pool_emit_draw_commands", "gv_pool_draw_commands_device",
    "gv_pool_draw_commands_fetch",
    "gv_pool_bind_clusters", "gv_pool_cull_clusters", "gv_pool_cluster_commands_device", "gv_pool_cluster_commands_fetch",
    "gv_pool_cull_clusters_second_phase", "gv_pool_cluster_second_commands_device", "gv_pool_cluster_second_commands_fetch",
    "gv_pool_cull_cluster_runs", "gv_pool_bind_cluster_cones", "gv_pool_cull_cluster_cones",
    "gv_pool_bind_cluster_lods", "gv_pool_cull_cluster_lods",
    "gv_pool_bind_lod", "gv_pool_select_lods", "gv_pool_lods_device", "gv_pool_lods_fetch",
    "gv_pool_group_draws",
    "gv_pool_cull_second_phase",
    "gv_pool_view_bounds", "gv_pool_view_bounds_device", "gv_pool_view_bounds_fetch",
    "gv_pool_view_delta", "gv_pool_view_delta_device", "gv_pool_view_delta_fetch",
    "gv_pool_bind_occluders", "gv_occluder_begin", "gv_pool_draw_occluders", "gv_occluder_depth_device", "gv_occluder_depth_fetch",
    "gv_hiz_build_from_occluders",
    "gv_pool_keep_models", "gv_pool_forget_models", "gv_pool_emit_previous", "gv_pool_previous_device", "gv_pool_previous_fetch",
    "gv_receiver_begin", "gv_pool_draw_receivers", "gv_receiver_mask_device", "gv_receiver_mask_fetch", "gv_hiz_build_from_receivers",
]

_lib = None


def load():
    """dlopen the HIP library (no compute). Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: build it with `make -C garden_amd/csrc` (or __graft_entry__.build()); "
            "there is no CPU fallback")
    # One HIP runtime per process: PyTorch bundles its own libamdhip64, and a process that loads the system one first
    # (through this library) and torch's second ends up with two runtimes, the second of which finds no GPU. Loading
    # torch's first makes this library bind to it as well (same SONAME). torch stays optional.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    P, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    lib.gv_abi_version.restype = u32
    lib.gv_create.argtypes = [C.POINTER(GvConfig), C.POINTER(P)]
    lib.gv_destroy.argtypes = [P]
    lib.gv_destroy.restype = None
    lib.gv_last_error.argtypes = [P]
    lib.gv_last_error.restype = C.c_char_p
    lib.gv_transform_bind.argtypes = [P, P, sz, u32, C.POINTER(GvTransformLayout), P, u32]
    lib.gv_pool_bind.argtypes = [P, u32, P, sz, u32, C.POINTER(GvMeshLayout)]
    lib.gv_transform_bind_columns.argtypes = [P, C.POINTER(GvTransformColumns), u32, P, u32]
    lib.gv_pool_bind_columns.argtypes = [P, u32, C.POINTER(GvMeshColumns), u32]
    lib.gv_pool_bind_ready.argtypes = [P, u32, P, u32, u32]
    lib.gv_mark_dirty.argtypes = [P, u32, u32, u32]
    lib.gv_hierarchy_rebuild.argtypes = [P]
    lib.gv_sync.argtypes = [P]
    lib.gv_cull.argtypes = [P, u32, C.POINTER(GvView), u32]
    lib.gv_wait.argtypes = [P]
    lib.gv_results_fetch.argtypes = [P, u32, C.c_int, C.POINTER(GvResult)]
    lib.gv_result_count.argtypes = [P, u32, C.POINTER(u32)]
    lib.gv_results_device.argtypes = [P, u32, C.POINTER(GvDeviceResult)]
    lib.gv_results_copy_idx_device.argtypes = [P, u32, P, u32, u32]
    lib.gv_results_copy_shard_device.argtypes = [P, u32, P, u32, u32]
    lib.gv_results_copy_mask_device.argtypes = [P, u32, P, u32]
    lib.gv_pool_mirror_slots.argtypes = [P, u32, P, u32]
    lib.gv_pool_mirror_epoch.argtypes = [P, u32, P]
    lib.gv_sort.argtypes = [P, u32, C.c_int]
    lib.gv_sweep.argtypes = [P, u32]
    lib.gv_get_world.argtypes = [P, u32, u32, P]
    lib.gv_hiz_build.argtypes = [P, P, u32, u32, u32]
    lib.gv_hiz_rebuild.argtypes = [P]
    lib.gv_hiz_read_level.argtypes = [P, u32, P, C.POINTER(u32), C.POINTER(u32)]
    lib.gv_hiz_mip_count.argtypes = [P, C.POINTER(u32)]
    lib.gv_hiz_select.argtypes = [P, u32]
    lib.gv_hiz_drop.argtypes = [P, u32]
    lib.gv_stats.argtypes = [P, C.POINTER(GvStats)]
    lib.gv_stats_reset.argtypes = [P]
    lib.gv_debug_stream_peak.argtypes = [P, u32, u32, C.POINTER(C.c_double)]
    lib.gv_stream.argtypes = [P]
    lib.gv_stream.restype = P
    lib.gv_scene_parse_json.argtypes = [C.c_char_p, sz, C.POINTER(GvScenePool), u32, u32, C.POINTER(P), C.c_char_p, sz]
    lib.gv_scene_parse_bson.argtypes = [C.c_char_p, sz, C.POINTER(GvScenePool), u32, u32, C.POINTER(P), C.c_char_p, sz]
    lib.gv_scene_destroy.argtypes = [P]
    lib.gv_scene_destroy.restype = None
    lib.gv_scene_info.argtypes = [P, C.POINTER(GvSceneInfo)]
    lib.gv_scene_transform_columns.argtypes = [P, C.POINTER(GvTransformColumns), C.POINTER(u32), C.POINTER(P),
                                               C.POINTER(u32), C.POINTER(P)]
    lib.gv_scene_mesh_columns.argtypes = [P, u32, C.POINTER(GvMeshColumns), C.POINTER(u32)]
    lib.gv_scene_bind.argtypes = [P, P]
    lib.gv_scene_extract_tile.argtypes = [P, C.POINTER(C.c_uint32 * 3), C.c_double, u32, C.POINTER(P)]
    lib.gv_scene_extract_rank.argtypes = [P, C.POINTER(C.c_uint32 * 3), C.c_double, u32, u32, C.POINTER(P)]
    lib.gv_cell_owner.argtypes = [C.POINTER(C.c_uint32 * 3), C.c_double, u32, P, u32, u32, P]
    lib.gv_scene_tile_maps.argtypes = [P, u32, C.POINTER(P), C.POINTER(u32), C.POINTER(P), C.POINTER(u32)]
    lib.gv_exchange_unique_id.argtypes = [P]
    lib.gv_exchange_init.argtypes = [P, P, C.c_int, C.c_int]
    lib.gv_exchange_shards.argtypes = [P, u32, u32, P, u32, P]
    lib.gv_exchange_visible.argtypes = [P, u32, u32, u32, C.POINTER(GvExchangeFrame)]
    lib.gv_exchange_acquire.argtypes = [P, C.c_uint64, C.POINTER(GvExchangeFrame)]
    lib.gv_exchange_init_all.argtypes = [C.POINTER(P), C.c_int]
    lib.gv_exchange_init_peers.argtypes = [C.POINTER(P), C.c_int]
    lib.gv_exchange_visible_all.argtypes = [C.POINTER(P), C.c_int, C.POINTER(u32), C.POINTER(u32), u32, C.POINTER(GvExchangeFrame)]
    lib.gv_pool_exchange_visible.argtypes = [P, u32, u32, u32, u32, C.POINTER(GvExchangeFrame)]
    lib.gv_pool_exchange_visible_all.argtypes = [C.POINTER(P), C.c_int, u32, C.POINTER(u32), C.POINTER(u32), u32, C.POINTER(GvExchangeFrame)]
    lib.gv_exchange_acquire_all.argtypes = [C.POINTER(P), C.c_int, C.c_uint64, C.POINTER(GvExchangeFrame)]
    lib.gv_exchange_views.argtypes = [P, C.POINTER(GvExchangeItem), u32, u32, C.POINTER(GvExchangeFrame)]
    lib.gv_exchange_views_all.argtypes = [C.POINTER(P), C.c_int, C.POINTER(GvExchangeItem), u32, u32, C.POINTER(GvExchangeFrame)]
    lib.gv_pool_update_index_map.argtypes = [P, u32, u32, C.POINTER(u32), u32]
    lib.gv_pool_set_result_mapping.argtypes = [P, u32, u32, C.c_void_p, C.c_size_t, u32]
    lib.gv_host_parallel_ranges.argtypes = [u32, u32, C.c_void_p, C.c_void_p]
    lib.gv_host_parallel_ranges.restype = None
    lib.gv_host_parallel_tasks.argtypes = [u32, C.c_void_p, C.c_void_p]
    lib.gv_host_parallel_tasks.restype = None
    lib.gv_exchange_set_timeout.argtypes = [P, u32]
    lib.gv_exchange_masks.argtypes = [P, u32, u32, P]
    lib.gv_exchange_shutdown.argtypes = [P]
    lib.gv_exchange_set_mode.argtypes = [P, u32]
    lib.gv_pool_set_index_map.argtypes = [P, u32, P, u32]
    lib.gv_pool_results_fetch.argtypes = [P, u32, u32, C.c_int, C.POINTER(GvResult)]
    lib.gv_pool_result_count.argtypes = [P, u32, u32, C.POINTER(u32)]
    lib.gv_pool_results_device.argtypes = [P, u32, u32, C.POINTER(GvDeviceResult)]
    lib.gv_pool_sort.argtypes = [P, u32, u32, C.c_int]
    lib.gv_pool_set_record_layout.argtypes = [P, u32, C.POINTER(GvRecordLayout)]
    lib.gv_pool_results_records.argtypes = [P, u32, u32, C.POINTER(C.c_void_p), C.POINTER(u32)]
    lib.gv_pool_set_record_target.argtypes = [P, u32, u32, C.c_void_p, C.c_size_t]
    lib.gv_profile_sampling.argtypes = [P, u32]
    lib.gv_profile_samples.argtypes = [P, C.POINTER(C.c_uint64 * GV_K_COUNT)]
    lib.gv_profile_kernels.argtypes = [P, u32]
    lib.gv_pool_results_instance_bases.argtypes = [P, u32, u32, C.POINTER(C.POINTER(u32)), C.POINTER(u32)]
    lib.gv_cull_batch_begin.argtypes = [P]
    lib.gv_cull_batch_end.argtypes = [P]
    lib.gv_pick.argtypes = [P, C.POINTER(u32), u32, C.POINTER(u32), C.POINTER(C.c_float), C.POINTER(GvPickRay), u32, C.POINTER(GvPickHit)]
    lib.gv_pool_set_instance_layout.argtypes = [P, u32, C.POINTER(GvInstanceLayout)]
    lib.gv_pool_emit_instances.argtypes = [P, u32, C.POINTER(u32), u32, P, sz]
    lib.gv_pool_instances_device.argtypes = [P, u32, C.POINTER(P), C.POINTER(P)]
    lib.gv_pool_instances_info.argtypes = [P, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    lib.gv_pool_instances_fetch.argtypes = [P, u32, P, sz, C.POINTER(u32), u32]
    lib.gv_pool_bind_payload.argtypes = [P, u32, C.POINTER(GvPayloadField), u32, u32]
    lib.gv_pool_set_payload_layout.argtypes = [P, u32, C.POINTER(u32), u32]
    lib.gv_pool_emit_draw_instances.argtypes = [P, u32, C.POINTER(u32), u32, P, sz]
    lib.gv_pool_set_instance_index_field.argtypes = [P, u32, u32]
    lib.gv_pool_draw_bases_device.argtypes = [P, u32, C.POINTER(P), C.POINTER(P)]
    lib.gv_pool_draw_bases_fetch.argtypes = [P, u32, C.POINTER(u32), u32, C.POINTER(u32), u32]
    lib.gv_merge_sorted.argtypes = [P, C.POINTER(GvMergeGroup), u32]
    lib.gv_merge_device.argtypes = [P, u32, C.POINTER(P), C.POINTER(P)]
    lib.gv_merge_fetch.argtypes = [P, u32, P, sz, C.POINTER(u32), u32]
    lib.gv_pool_bind_geometry.argtypes = [P, u32, P, u32, u32, u32, C.POINTER(GvGeometry), u32]
    lib.gv_pool_set_command_layout.argtypes = [P, u32, C.POINTER(GvCommandLayout)]
    lib.gv_pool_emit_draw_commands.argtypes = [P, u32, u32, u32, P, sz]
    lib.gv_pool_draw_commands_device.argtypes = [P, u32, C.POINTER(P), C.POINTER(P)]
    lib.gv_pool_draw_commands_fetch.argtypes = [P, u32, P, sz, C.POINTER(u32), u32]
    lib.gv_pool_bind_clusters.argtypes = [P, u32, C.POINTER(GvClusterRange), u32, C.POINTER(GvCluster), u32]
    lib.gv_pool_cull_clusters.argtypes = [P, u32, u32, u32, P, sz]
    lib.gv_pool_cluster_commands_device.argtypes = [P, u32, C.POINTER(P), C.POINTER(P)]
    lib.gv_pool_cluster_commands_fetch.argtypes = [P, u32, P, sz, C.POINTER(u32), u32]
    lib.gv_pool_cull_clusters_second_phase.argtypes = [P, u32, u32, u32, P, sz]
    lib.gv_pool_cluster_second_commands_device.argtypes = [P, u32, C.POINTER(P), C.POINTER(P)]
    lib.gv_pool_cluster_second_commands_fetch.argtypes = [P, u32, P, sz, C.POINTER(u32), u32]
    lib.gv_pool_cull_cluster_runs.argtypes = [P, u32, u32, u32, P, sz]
    lib.gv_pool_bind_cluster_cones.argtypes = [P, u32, P, u32]
    lib.gv_pool_cull_cluster_cones.argtypes = [P, u32, u32, P, u32, u32, P, sz]
    lib.gv_pool_bind_cluster_lods.argtypes = [P, u32, P, u32]
    lib.gv_pool_cull_cluster_lods.argtypes = [P, u32, u32, P, u32, P, u32, u32, P, sz]
    lib.gv_pool_bind_lod.argtypes = [P, u32, P, u32, u32, C.POINTER(GvLodGeometry), u32]
    lib.gv_pool_select_lods.argtypes = [P, u32, C.POINTER(C.c_float), u32]
    lib.gv_pool_lods_device.argtypes = [P, u32, C.POINTER(P), C.POINTER(P)]
    lib.gv_pool_lods_fetch.argtypes = [P, u32, C.POINTER(u32), u32, C.POINTER(u32), u32]
    lib.gv_pool_group_draws.argtypes = [P, u32, u32, u32, C.c_float]
    lib.gv_pool_cull_second_phase.argtypes = [P, u32, u32, u32, C.POINTER(GvView)]
    lib.gv_pool_view_bounds.argtypes = [P, u32, C.POINTER(u32), C.POINTER(C.c_float), u32]
    lib.gv_pool_view_bounds_device.argtypes = [P, u32, C.POINTER(P), C.POINTER(u32)]
    lib.gv_pool_view_bounds_fetch.argtypes = [P, u32, C.POINTER(GvViewBounds), u32]
    lib.gv_pool_view_delta.argtypes = [P, u32, u32, C.POINTER(u32), u32, u32]
    lib.gv_pool_view_delta_device.argtypes = [P, u32, u32, C.POINTER(P), C.POINTER(P)]
    lib.gv_pool_view_delta_fetch.argtypes = [P, u32, u32, C.c_int, C.POINTER(GvViewDelta)]
    lib.gv_pool_bind_occluders.argtypes = [P, u32, P, P, u32, u32]
    lib.gv_occluder_begin.argtypes = [P, u32, u32]
    lib.gv_pool_draw_occluders.argtypes = [P, u32, u32, u32]
    lib.gv_occluder_depth_device.argtypes = [P, C.POINTER(P), C.POINTER(u32), C.POINTER(u32), C.POINTER(P)]
    lib.gv_occluder_depth_fetch.argtypes = [P, P, C.c_size_t, C.POINTER(GvOccluderCounts)]
    lib.gv_hiz_build_from_occluders.argtypes = [P]
    lib.gv_pool_keep_models.argtypes = [P, u32, u32, u32]
    lib.gv_pool_forget_models.argtypes = [P, u32, u32, u32]
    lib.gv_pool_emit_previous.argtypes = [P, u32, u32, C.POINTER(GvPreviousLayout), C.POINTER(C.c_float), u32, P, C.c_size_t]
    lib.gv_pool_previous_device.argtypes = [P, u32, C.POINTER(P), C.POINTER(P)]
    lib.gv_pool_previous_fetch.argtypes = [P, u32, P, C.c_size_t, C.POINTER(u32)]
    lib.gv_receiver_begin.argtypes = [P, u32, u32]
    lib.gv_pool_draw_receivers.argtypes = [P, u32, u32, P]
    lib.gv_receiver_mask_device.argtypes = [P, C.POINTER(P), C.POINTER(u32), C.POINTER(u32), C.POINTER(P)]
    lib.gv_receiver_mask_fetch.argtypes = [P, P, C.c_size_t, C.POINTER(GvReceiverCounts)]
    lib.gv_hiz_build_from_receivers.argtypes = [P]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name not in ("gv_abi_version", "gv_destroy", "gv_last_error", "gv_stream", "gv_scene_destroy"):
            fn.restype = C.c_int
    _lib = lib
    return lib


def to_gv_view(v):
    out = GvView()
    out.view_proj[:] = [float(x) for x in v["view_proj"]]
    out.camera_position[:] = [float(x) for x in v["camera_position"]]
    out.camera_offset[:] = [float(x) for x in v["camera_offset"]]
    out.shadow_pass = v.get("shadow_pass", -1)
    out.use_hiz = v.get("use_hiz", 0)
    out.distance_2d = v.get("distance_2d", 0)
    out.emit_records = v.get("emit_records", 1)
    return out


class GpuVisibility:
    """One libgarden_vis context (one per process per GPU). Thin: every method is one C-ABI call."""

    def __init__(self, device=0, hiz_rule=GV_HIZ_RULE_REFERENCE, profile_events=False, profile_cull_only=False,
                 keep_slot_order=False, block_bounds=False, hiz_rg16f=False, linear_scan=False):
        self.lib = load()
        flags = GV_CONFIG_PROFILE_EVENTS if (profile_events or profile_cull_only) else 0
        if profile_cull_only:
            flags |= GV_CONFIG_PROFILE_CULL_ONLY
        if keep_slot_order:
            flags |= GV_CONFIG_KEEP_SLOT_ORDER
        if block_bounds:
            flags |= GV_CONFIG_BLOCK_BOUNDS
        if hiz_rg16f:
            flags |= GV_CONFIG_HIZ_RG16F
        if linear_scan:
            flags |= GV_CONFIG_LINEAR_SCAN
        cfg = GvConfig(C.sizeof(GvConfig), device, hiz_rule, flags)
        self.ctx = C.c_void_p()
        rc = self.lib.gv_create(C.byref(cfg), C.byref(self.ctx))
        if rc != GV_OK:
            self.ctx = C.c_void_p()
            raise GvError(rc, self.lib.gv_last_error(None).decode())
        self._keep = {}

    def close(self):
        if getattr(self, "ctx", None) and self.ctx.value:
            self.lib.gv_destroy(self.ctx)
            self.ctx = C.c_void_p()
            self._keep = {}  # bound pools and record targets are let go only after the context (and its page locks) is gone

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != GV_OK:
            raise GvError(rc, self.lib.gv_last_error(self.ctx).decode())

    # ---- binding ----
    def bind_transforms(self, transforms, entity_to_transform):
        lay = GvTransformLayout(**transform_layout_offsets(transforms.dtype))
        e2t = np.ascontiguousarray(entity_to_transform, dtype=np.uint32)
        self._keep["xf"] = (transforms, e2t)
        self._check(self.lib.gv_transform_bind(self.ctx, transforms.ctypes.data, transforms.dtype.itemsize,
                                               transforms.shape[0], C.byref(lay), e2t.ctypes.data, e2t.shape[0]))

    def bind_pool(self, pool_id, meshes):
        lay = GvMeshLayout(**mesh_layout_offsets(meshes.dtype))
        self._keep[("pool", pool_id)] = meshes
        self._check(self.lib.gv_pool_bind(self.ctx, pool_id, meshes.ctypes.data, meshes.dtype.itemsize,
                                          meshes.shape[0], C.byref(lay)))

    @staticmethod
    def _column(a):
        """GvColumn of a numpy array whose rows are the elements (C-contiguous rows; any row stride)."""
        assert a.ndim in (1, 2) and (a.ndim == 1 or a.strides[1] == a.itemsize)
        return GvColumn(a.ctypes.data, a.strides[0])

    def bind_transform_columns(self, columns, entity_to_transform):
        """columns: dict of numpy arrays entity/parent (u32[n]), position/scale (f32[n,3+]), rotation (f32[n,4]),
        self_active/ancestors_active/model_with_ancestors (u8[n]). The caller keeps them alive and unmoved."""
        self._xf_columns, self._e2t = columns, np.ascontiguousarray(entity_to_transform, dtype=np.uint32)
        c = GvTransformColumns(*[self._column(columns[n]) for n, _ in GvTransformColumns._fields_])
        self._check(self.lib.gv_transform_bind_columns(self.ctx, C.byref(c), columns["entity"].shape[0],
                                                       self._e2t.ctypes.data, self._e2t.shape[0]))

    def bind_pool_columns(self, pool_id, columns):
        """columns: dict of numpy arrays entity (u32[n]), is_enabled (u8[n]), aabb_min/aabb_max (f32[n,3+]) and
        optionally is_visible (u8[n], written by fetch(write_back=True))."""
        self._pool_columns = getattr(self, "_pool_columns", {})
        self._pool_columns[pool_id] = columns
        vis = columns.get("is_visible")
        c = GvMeshColumns(self._column(columns["entity"]), self._column(columns["is_enabled"]),
                          self._column(columns["aabb_min"]), self._column(columns["aabb_max"]),
                          vis.ctypes.data if vis is not None else None, vis.strides[0] if vis is not None else 0)
        self._check(self.lib.gv_pool_bind_columns(self.ctx, pool_id, C.byref(c), columns["entity"].shape[0]))

    def bind_ready(self, pool_id, ready):
        """Per-slot ready counts of `pool_id` (numpy u8 or u32 array, one element per slot; None removes the column)."""
        if ready is None:
            self._keep.pop(("ready", pool_id), None)
            self._check(self.lib.gv_pool_bind_ready(self.ctx, pool_id, None, 0, 0))
            return
        assert ready.dtype in (np.uint8, np.uint32) and ready.ndim == 1
        self._keep[("ready", pool_id)] = ready
        self._check(self.lib.gv_pool_bind_ready(self.ctx, pool_id, ready.ctypes.data, ready.strides[0], ready.dtype.itemsize))

    def mark_dirty(self, kind, first, count, pool_id=0):
        if kind in (GV_DIRTY_MESH, GV_DIRTY_PAYLOAD, GV_DIRTY_GEOMETRY, GV_DIRTY_LOD, GV_DIRTY_OCCLUDER):
            first |= pool_id << 28
        self._check(self.lib.gv_mark_dirty(self.ctx, kind, first, count))

    def hierarchy_rebuild(self):
        self._check(self.lib.gv_hierarchy_rebuild(self.ctx))

    def sync(self):
        self._check(self.lib.gv_sync(self.ctx))

    # ---- per frame ----
    def cull(self, pool_id, views):
        """views: a list of view dicts (scene.make_view), or the array views_array() made of one (a frame loop that
        re-submits the same views need not rebuild the ctypes structs every frame)."""
        arr = views if isinstance(views, C.Array) else self.views_array(views)
        self._check(self.lib.gv_cull(self.ctx, pool_id, arr, len(arr)))
        self._culled_pool = pool_id

    @staticmethod
    def views_array(views):
        return (GvView * len(views))(*[to_gv_view(v) for v in views])

    def cull_batch_begin(self):
        """Culls of small pools are recorded until the first read and then launched together (one tick, four launches)."""
        self._check(self.lib.gv_cull_batch_begin(self.ctx))

    def cull_batch_end(self):
        self._check(self.lib.gv_cull_batch_end(self.ctx))

    def wait(self):
        self._check(self.lib.gv_wait(self.ctx))

    def result_count(self, view_index=0):
        n = C.c_uint32()
        self._check(self.lib.gv_result_count(self.ctx, view_index, C.byref(n)))
        return n.value

    def fetch(self, view_index=0, write_back=True, occupancy=None, order="slot", pool_id=None):
        """Returns copies: dict(visible_idx, baked_model[n,12], distance_sq, is_visible or None, draw_count).
        order="slot": records re-ordered here by pool slot (what the oracle's single-thread loop produces);
        order="raw": as the library emitted them (mirror order, or distance order after sort()).
        pool_id: the pool whose results are read (default: the pool of the most recent cull)."""
        r = GvResult()
        if pool_id is None:
            self._check(self.lib.gv_results_fetch(self.ctx, view_index, 1 if write_back else 0, C.byref(r)))
        else:
            self._check(self.lib.gv_pool_results_fetch(self.ctx, pool_id, view_index, 1 if write_back else 0, C.byref(r)))
        n = r.draw_count
        out = dict(draw_count=n, instance_count=r.instance_count, visible_idx=None, baked_model=None,
                   distance_sq=None, is_visible=None)
        if n and r.visible_idx:
            out["visible_idx"] = np.ctypeslib.as_array(r.visible_idx, shape=(n,)).copy()
            out["baked_model"] = np.ctypeslib.as_array(r.baked_model, shape=(n, 12)).copy()
            out["distance_sq"] = np.ctypeslib.as_array(r.distance_sq, shape=(n,)).copy()
            if order == "slot":
                o = np.argsort(out["visible_idx"], kind="stable")
                out["visible_idx"], out["baked_model"], out["distance_sq"] = \
                    out["visible_idx"][o], out["baked_model"][o], out["distance_sq"][o]
        elif n == 0:
            out["visible_idx"] = np.zeros(0, np.uint32)
            out["baked_model"] = np.zeros((0, 12), np.float32)
            out["distance_sq"] = np.zeros(0, np.float32)
        if r.is_visible and occupancy:
            out["is_visible"] = np.ctypeslib.as_array(r.is_visible, shape=(occupancy,)).copy()
        return out

    def set_record_layout(self, pool_id, dtype=None, component_stride=1, buffer_index_value=0):
        """Deliver pool `pool_id`'s records as an array of structs described by the numpy structured `dtype` with fields
        componentOffset (u8), bakedModel (12 x f4), distanceSq (f4) and optionally bufferIndex (u4); None removes it."""
        if dtype is None:
            self._check(self.lib.gv_pool_set_record_layout(self.ctx, pool_id, None))
            return
        dtype = np.dtype(dtype)
        at = {name: dtype.fields[name][1] for name in dtype.names}
        layout = GvRecordLayout(dtype.itemsize, at["componentOffset"], at["bakedModel"], at["distanceSq"],
                                at.get("bufferIndex", 0xFFFFFFFF), component_stride, buffer_index_value)
        self._check(self.lib.gv_pool_set_record_layout(self.ctx, pool_id, C.byref(layout)))

    def records(self, pool_id, view_index, dtype):
        """The fetched records of (pool, view) as a copy of the library's struct array, viewed as `dtype`."""
        ptr, n = C.c_void_p(), C.c_uint32()
        self._check(self.lib.gv_pool_results_records(self.ctx, pool_id, view_index, C.byref(ptr), C.byref(n)))
        dtype = np.dtype(dtype)
        if n.value == 0:
            return np.zeros(0, dtype)
        raw = (C.c_uint8 * (n.value * dtype.itemsize)).from_address(ptr.value)
        return np.frombuffer(raw, dtype=np.uint8).copy().view(dtype)  # bytewise: a structured copy would skip the padding

    def set_record_target(self, pool_id, view_index, array):
        """The records of (pool, view) are written straight into `array` (a C-contiguous numpy array the caller keeps alive
        and in place; None removes the target): the engine's own combinedMeshes instead of the library's buffer."""
        if array is None:
            self._check(self.lib.gv_pool_set_record_target(self.ctx, pool_id, view_index, None, 0))
            self._keep.pop(("target", pool_id, view_index), None)  # (only now: the call above checks that the range is still mapped)
            return
        assert array.flags["C_CONTIGUOUS"] and array.flags["WRITEABLE"]
        self._check(self.lib.gv_pool_set_record_target(self.ctx, pool_id, view_index, array.ctypes.data, array.nbytes))
        self._keep[("target", pool_id, view_index)] = array  # the fetch copies the records into it (never page-locked) until replaced / removed / close()

    def instance_bases(self, pool_id=0, view_index=0):
        """First instance index of every fetched record ([count + 1] words; the last one is instance_count)."""
        ptr, n = C.POINTER(C.c_uint32)(), C.c_uint32()
        self._check(self.lib.gv_pool_results_instance_bases(self.ctx, pool_id, view_index, C.byref(ptr), C.byref(n)))
        return np.ctypeslib.as_array(ptr, shape=(n.value + 1,)).copy()

    def results_device(self, view_index=0):
        d = GvDeviceResult()
        self._check(self.lib.gv_results_device(self.ctx, view_index, C.byref(d)))
        return d

    def set_index_map(self, pool_id, global_ids):
        """Pool slot -> global id table for the exchange shards of `pool_id` (None / empty removes it)."""
        if global_ids is None or len(global_ids) == 0:
            self._check(self.lib.gv_pool_set_index_map(self.ctx, pool_id, None, 0))
            return
        g = np.ascontiguousarray(global_ids, dtype=np.uint32)
        self._check(self.lib.gv_pool_set_index_map(self.ctx, pool_id, g.ctypes.data, g.shape[0]))

    def copy_idx_device(self, view_index, dst_ptr, capacity, index_base=0):
        self._check(self.lib.gv_results_copy_idx_device(self.ctx, view_index, dst_ptr, capacity, index_base))

    def copy_shard_device(self, view_index, dst_ptr, capacity, index_base=0):
        """dst[0] = draw_count, dst[1:1+min(count, capacity)] = visible_idx + index_base (device memory, no sync)."""
        self._check(self.lib.gv_results_copy_shard_device(self.ctx, view_index, dst_ptr, capacity, index_base))

    def copy_mask_device(self, view_index, dst_ptr, word_count):
        """Exchange shard as a bit per MIRROR entry: [draw_count, ceil(occupancy / 32) words] into device memory at dst_ptr
        (entry e is pool slot mirror_slots()[e])."""
        self._check(self.lib.gv_results_copy_mask_device(self.ctx, view_index, dst_ptr, word_count))

    def mirror_epoch(self, pool_id=0):
        """Changes whenever mirror_slots() does (rebuild, appended slots, re-order after entity churn)."""
        e = C.c_uint64()
        self._check(self.lib.gv_pool_mirror_epoch(self.ctx, pool_id, C.byref(e)))
        return int(e.value)

    def mirror_slots(self, pool_id, occupancy):
        """entry -> pool slot table of the pool's device mirror (changes only when the mirror is rebuilt)."""
        out = np.empty(occupancy, dtype=np.uint32)
        self._check(self.lib.gv_pool_mirror_slots(self.ctx, pool_id, out.ctypes.data, occupancy))
        return out

    # ---- native RCCL exchange (what a C++ engine calls; bench.py --gpus N times it: config.exchange_path "c-abi") ----
    @staticmethod
    def exchange_unique_id():
        buf = C.create_string_buffer(128)
        rc = load().gv_exchange_unique_id(buf)
        if rc != GV_OK:
            raise GvError(rc, "gv_exchange_unique_id failed (RCCL not loadable?)")
        return buf.raw

    def exchange_init(self, unique_id, rank, world_size):
        self._check(self.lib.gv_exchange_init(self.ctx, unique_id, rank, world_size))

    def exchange_shards(self, view_index, capacity, index_base, gathered_ptr, capacities=None, world=None):
        """Caller-owned rows [world, 1 + capacity]; capacities (one per rank, the same list on every rank): what of each
        rank's row travels under the direct patterns. (gv_exchange_shards reads one capacity per rank of the communicator: pass
        `world` to have the list's length checked here.)"""
        caps = None
        if capacities is not None:
            if world is not None and len(capacities) != world:
                raise ValueError(f"exchange_shards: {len(capacities)} capacities for {world} ranks")
            caps = (C.c_uint32 * max(len(capacities), GV_EXCHANGE_MAX_RANKS))(*[int(c) for c in capacities])
        self._check(self.lib.gv_exchange_shards(self.ctx, view_index, capacity, caps, index_base, gathered_ptr))

    @staticmethod
    def _exchange_frame(f):
        w = f.world_size
        return dict(ptr=f.gathered_device, row_words=f.row_words, world=w, frame=int(f.frame), complete=bool(f.complete),
                    room=[int(f.room[r]) for r in range(w)], travelled_words=[int(f.travelled_words[r]) for r in range(w)],
                    counts=[int(f.counts[r]) for r in range(w)], tail_words=[int(f.tail_words[r]) for r in range(w)],
                    cut_ranks=[r for r in range(w) if (f.cut_ranks >> r) & 1], mode=int(f.mode), ready_event=f.ready_event,
                    # gv_exchange_views: lists per rank in the frame (0: a single-list frame) and, once acquired, item_counts[r][i]
                    items=int(f.items), item_counts=([[int(f.item_counts[r * f.items + i]) for i in range(f.items)] for r in range(w)]
                                                     if f.items and f.item_counts else None))

    def exchange_visible(self, view_index=0, index_base=0, pool_id=None):
        """Sends the frame (gv_exchange_visible; pool_id: gv_pool_exchange_visible for a named pool): library-owned rows, sized from
        the previous frame's headers. Returns a dict: frame, row_words, world, room, travelled_words, mode — the rows themselves are
        handed out by exchange_acquire."""
        f = GvExchangeFrame()
        if pool_id is None:
            self._check(self.lib.gv_exchange_visible(self.ctx, view_index, index_base, 0, C.byref(f)))
        else:
            self._check(self.lib.gv_pool_exchange_visible(self.ctx, pool_id, view_index, index_base, 0, C.byref(f)))
        return self._exchange_frame(f)

    def exchange_views(self, items):
        """ONE exchange for ALL the lists of a frame (gv_exchange_views): items = [(pool_id, view_index, index_base), ...], the same
        list on every rank. Row r of the acquired frame = [len(items) + total, c_0 .. c_k, list 0, list 1 ...]."""
        arr = (GvExchangeItem * len(items))(*[GvExchangeItem(int(p), int(v), int(b)) for p, v, b in items])
        f = GvExchangeFrame()
        self._check(self.lib.gv_exchange_views(self.ctx, arr, len(items), 0, C.byref(f)))
        return self._exchange_frame(f)

    def update_index_map(self, pool_id, first, global_ids):
        ids = np.ascontiguousarray(global_ids, dtype=np.uint32)
        self._check(self.lib.gv_pool_update_index_map(self.ctx, pool_id, int(first), ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.shape[0]))

    def set_result_mapping(self, pool_id, flags, visible=None, stride=1):
        """gv_pool_set_result_mapping: records in world slots (GV_RESULTS_MAP_RECORDS) and / or the write-back of isVisible through the
        index map into `visible` (a uint8 array the caller keeps alive; element i at visible + i * stride)."""
        base = visible.ctypes.data if visible is not None else None
        count = (visible.nbytes // stride) if visible is not None else 0
        self._check(self.lib.gv_pool_set_result_mapping(self.ctx, pool_id, int(flags), base, int(stride), int(count)))

    def exchange_acquire(self, frame):
        """Frame `frame` complete — every rank's WHOLE list, short predictions made good by a second exchange — and the context's
        stream ordered behind it (gv_exchange_acquire). Returns the frame's dict: ptr (device address of the uint32 rows
        [world, row_words]), counts, cut_ranks / tail_words (statistics), ready_event."""
        f = GvExchangeFrame()
        self._check(self.lib.gv_exchange_acquire(self.ctx, frame, C.byref(f)))
        return self._exchange_frame(f)

    def exchange_set_timeout(self, milliseconds):
        self._check(self.lib.gv_exchange_set_timeout(self.ctx, milliseconds))

    def exchange_masks(self, view_index, word_count, gathered_ptr):
        """All ranks' [draw_count, one bit per mirror entry] shards into gathered_ptr ([world, 1 + word_count] uint32, device)."""
        self._check(self.lib.gv_exchange_masks(self.ctx, view_index, word_count, gathered_ptr))

    def exchange_set_mode(self, mode):
        """0 all-gather, 1 grouped send/recv with every peer, 2 one broadcast per root (GvExchangeMode)."""
        self._check(self.lib.gv_exchange_set_mode(self.ctx, mode))

    def exchange_shutdown(self):
        self._check(self.lib.gv_exchange_shutdown(self.ctx))

    def stream(self):
        """The context's hipStream_t as an integer (e.g. for torch.cuda.ExternalStream)."""
        return self.lib.gv_stream(self.ctx)

    def sort(self, view_index=0, descending=False, pool_id=None):
        if pool_id is None:
            self._check(self.lib.gv_sort(self.ctx, view_index, 1 if descending else 0))
        else:
            self._check(self.lib.gv_pool_sort(self.ctx, pool_id, view_index, 1 if descending else 0))

    def group_draws(self, view_index=0, pool_id=None, by_lod=False, view_scale=1.0):
        """gv_pool_group_draws: the view's records reordered by geometry id (by_lod: by id + the level view_scale selects), stable,
        on the context's stream; the next fetch, emission or selection sees the new order. Call it before the pool's instance
        emission. pool_id: default, the pool of the most recent cull."""
        if pool_id is None:
            pool_id = getattr(self, "_culled_pool", 0)
        self._check(self.lib.gv_pool_group_draws(self.ctx, pool_id, view_index, GV_GROUP_BY_LOD if by_lod else 0, float(view_scale)))

    def cull_second_phase(self, first_view, second_view, view, pool_id=None):
        """gv_pool_cull_second_phase: the second phase of two-phase occlusion culling. Culls the pool with `view` (a view dict or
        a GvView) against the pyramid as it stands and leaves in `second_view` the records whose slot the records of `first_view`
        do not hold: an ordinary emitted view, on the context's stream. Its is_visible (main pass) is the union of both phases.
        pool_id: default, the pool of the most recent cull."""
        if pool_id is None:
            pool_id = getattr(self, "_culled_pool", 0)
        gv = view if isinstance(view, GvView) or view is None else to_gv_view(view)
        self._check(self.lib.gv_pool_cull_second_phase(self.ctx, pool_id, first_view, second_view, None if gv is None else C.byref(gv)))

    def view_bounds(self, pool_id, views, bases):
        """gv_pool_view_bounds + gv_pool_view_bounds_fetch: the bounds of the draws of each listed view in its basis (bases: 12
        float32 per item, c0.xyz c1.xyz c2.xyz c3.xyz; shape [items, 12] or [items, 4, 3]). Waits; returns a BOUNDS_DTYPE array,
        one element per item."""
        self.view_bounds_issue(pool_id, views, bases)
        return self.view_bounds_fetch(pool_id, len(np.asarray(views).reshape(-1)))

    def view_bounds_issue(self, pool_id, views, bases):
        """gv_pool_view_bounds alone: asynchronous on the context's stream"""
        v = np.ascontiguousarray(views, dtype=np.uint32).reshape(-1)
        b = np.ascontiguousarray(bases, dtype=np.float32).reshape(-1)
        if len(b) != 12 * len(v):
            raise ValueError(f"view_bounds: {len(v)} views with {len(b)} basis floats (12 per item)")
        self._check(self.lib.gv_pool_view_bounds(self.ctx, pool_id, v.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 b.ctypes.data_as(C.POINTER(C.c_float)), len(v)))

    def view_bounds_fetch(self, pool_id, capacity=GV_MAX_BOUNDS_ITEMS):
        """gv_pool_view_bounds_fetch: waits; the items of the pool's last gv_pool_view_bounds as a BOUNDS_DTYPE array"""
        out = np.zeros(max(int(capacity), 1), BOUNDS_DTYPE)
        self._check(self.lib.gv_pool_view_bounds_fetch(self.ctx, pool_id, out.ctypes.data_as(C.POINTER(GvViewBounds)), int(capacity)))
        return out[:self.view_bounds_device(pool_id)[1]]

    def view_bounds_device(self, pool_id):
        """gv_pool_view_bounds_device: (device pointer of GvViewBounds[items], items) of the pool's last gv_pool_view_bounds"""
        ptr, items = C.c_void_p(), C.c_uint32()
        self._check(self.lib.gv_pool_view_bounds_device(self.ctx, pool_id, C.byref(ptr), C.byref(items)))
        return ptr.value, int(items.value)

    # ---- what came into view and what left it ----
    def view_delta(self, pool_id, views, channel=0, restart=False, write_back=False):
        """gv_pool_view_delta + gv_pool_view_delta_fetch: the pool slots the listed views hold now and the channel's last call did not
        (appeared), and the other way round (vanished), ascending each. Waits; returns copies: dict(appeared, vanished,
        visible_count, slots). write_back: 1 / 0 into the isVisible bytes of exactly those slots (the bytes must have held the
        channel's baseline before)."""
        self.view_delta_issue(pool_id, views, channel, restart)
        return self.view_delta_fetch(pool_id, channel, write_back)

    def view_delta_issue(self, pool_id, views, channel=0, restart=False):
        """gv_pool_view_delta alone: asynchronous on the context's stream; commits the current set as the channel's baseline"""
        v = np.ascontiguousarray(views, dtype=np.uint32).reshape(-1)
        if len(v) == 0:
            raise ValueError("view_delta: no views (view_delta_drop drops a channel)")
        self._check(self.lib.gv_pool_view_delta(self.ctx, pool_id, channel, v.ctypes.data_as(C.POINTER(C.c_uint32)), len(v),
                                                GV_DELTA_RESTART if restart else 0))

    def view_delta_fetch(self, pool_id, channel=0, write_back=False):
        """gv_pool_view_delta_fetch: waits; the channel's last answer as copies"""
        d = GvViewDelta()
        self._check(self.lib.gv_pool_view_delta_fetch(self.ctx, pool_id, channel, 1 if write_back else 0, C.byref(d)))
        a, v = int(d.appeared_count), int(d.vanished_count)
        return dict(appeared=np.ctypeslib.as_array(d.appeared, shape=(a,)).copy() if a else np.zeros(0, np.uint32),
                    vanished=np.ctypeslib.as_array(d.vanished, shape=(v,)).copy() if v else np.zeros(0, np.uint32),
                    visible_count=int(d.visible_count), slots=int(d.slots))

    def view_delta_device(self, pool_id, channel=0):
        """gv_pool_view_delta_device: (device pointer of the slot words, device pointer of the four counts) of the channel's last answer"""
        slots, counts = C.c_void_p(), C.c_void_p()
        self._check(self.lib.gv_pool_view_delta_device(self.ctx, pool_id, channel, C.byref(slots), C.byref(counts)))
        return slots.value, counts.value

    def view_delta_drop(self, pool_id, channel=0):
        """gv_pool_view_delta(NULL, 0): the channel's baseline and result are dropped; its next call behaves as a first call"""
        self._check(self.lib.gv_pool_view_delta(self.ctx, pool_id, channel, None, 0, 0))

    # ---- picking ----
    def pick(self, rays, pool_ids=(0,), camera_position=(0, 0, 0), exclude=None):
        """gv_pick: rays = up to GV_MAX_PICK_RAYS (origin xyz, direction xyz) pairs, camera-relative (an array of shape [R, 2, 3]
        or [R, 6] works too); exclude = one slot per pool (None / GV_NONE: none). One (pool_id, slot, distance_sq) or None per ray."""
        r = np.asarray(rays, dtype=np.float32).reshape(-1, 6)
        arr = (GvPickRay * max(len(r), 1))()
        for k, row in enumerate(r):
            arr[k].origin[:3] = [float(x) for x in row[:3]]
            arr[k].direction[:3] = [float(x) for x in row[3:]]
        ids = (C.c_uint32 * max(len(pool_ids), 1))(*[int(p) for p in pool_ids])
        ex = None
        if exclude is not None:
            if len(exclude) != len(pool_ids):
                raise ValueError(f"pick: {len(exclude)} excluded slots for {len(pool_ids)} pools (one per pool, None: none)")
            ex = (C.c_uint32 * max(len(pool_ids), 1))(*[GV_NONE if e is None else int(e) for e in exclude])
        cam = (C.c_float * 4)(*[float(x) for x in list(camera_position)[:3]], 0.0)
        hits = (GvPickHit * max(len(r), 1))()
        self._check(self.lib.gv_pick(self.ctx, ids, len(pool_ids), ex, cam, arr, len(r), hits))
        return [None if hits[k].pool_id == GV_NONE else (int(hits[k].pool_id), int(hits[k].slot), float(hits[k].distance_sq))
                for k in range(len(r))]

    # ---- instance data ----
    def set_instance_layout(self, pool_id, stride=64, mvp=0, model=None, slot=None, distance_sq=None, dtype=None):
        """gv_pool_set_instance_layout: the plugin's instance struct, by offsets (None: the struct has no such field) or as a numpy
        structured `dtype` with the fields mvp (16 x f4) and optionally model (12 x f4), slot (u4), distanceSq (f4).
        stride=None removes the layout."""
        if dtype is not None:
            dtype = np.dtype(dtype)
            at = {name: dtype.fields[name][1] for name in dtype.names}
            stride, mvp, model, slot, distance_sq = dtype.itemsize, at["mvp"], at.get("model"), at.get("slot"), at.get("distanceSq")
        if stride is None:
            self._check(self.lib.gv_pool_set_instance_layout(self.ctx, pool_id, None))
            return
        none = lambda x: GV_NONE if x is None else int(x)
        layout = GvInstanceLayout(int(stride), int(mvp), none(model), none(slot), none(distance_sq))
        self._check(self.lib.gv_pool_set_instance_layout(self.ctx, pool_id, C.byref(layout)))

    def bind_payload(self, pool_id, arrays):
        """gv_pool_bind_payload: the component bytes the pool's instances carry next to mvp, one numpy array per field (at most 4):
        row i of an array is slot i's element — C-contiguous rows of 4 .. 64 bytes (a multiple of 4), any row stride, so a field of
        a structured (AoS) component array works as it is. All arrays have one row per slot. None or [] removes the payload. The
        caller keeps the arrays alive and unmoved until the calls that upload (sync / cull / emit_instances) have run."""
        arrays = list(arrays) if arrays is not None else []
        if not arrays:
            self._keep.pop(("payload", pool_id), None)
            self._check(self.lib.gv_pool_bind_payload(self.ctx, pool_id, None, 0, 0))
            return
        fields = (GvPayloadField * len(arrays))()
        for f, a in zip(fields, arrays):
            width = a.dtype.itemsize
            for dim, step in zip(a.shape[:0:-1], a.strides[:0:-1]):  # the rows themselves are C-contiguous
                assert step == width
                width *= dim
            assert a.shape[0] == arrays[0].shape[0]
            f.data, f.stride, f.bytes = a.ctypes.data, a.strides[0], width
        self._keep[("payload", pool_id)] = arrays
        self._check(self.lib.gv_pool_bind_payload(self.ctx, pool_id, fields, len(arrays), arrays[0].shape[0]))

    def set_payload_layout(self, pool_id, at):
        """gv_pool_set_payload_layout: the offset of every payload field in the instance (None: mirrored, not written)."""
        arr = (C.c_uint32 * max(len(at), 1))(*[GV_NONE if x is None else int(x) for x in at])
        self._check(self.lib.gv_pool_set_payload_layout(self.ctx, pool_id, arr, len(at)))

    def emit_instances(self, pool_id, views, device=None):
        """gv_pool_emit_instances: the instance data of the listed views of `pool_id`, back to back, on the context's stream.
        device: None for the library's own buffer, or (device pointer, capacity in bytes) of caller-owned device memory."""
        idx = (C.c_uint32 * max(len(views), 1))(*[int(v) for v in views])
        ptr, cap = (None, 0) if device is None else (int(device[0]), int(device[1]))
        self._check(self.lib.gv_pool_emit_instances(self.ctx, pool_id, idx, len(views), ptr, cap))

    def emit_draw_instances(self, pool_id, views, device=None):
        """gv_pool_emit_draw_instances: like emit_instances, but every draw takes its ready count (bind_ready) of instances, read from
        the count mirror on the device; instances_info / instances_device / instances then describe this emission."""
        idx = (C.c_uint32 * max(len(views), 1))(*[int(v) for v in views])
        ptr, cap = (None, 0) if device is None else (int(device[0]), int(device[1]))
        self._check(self.lib.gv_pool_emit_draw_instances(self.ctx, pool_id, idx, len(views), ptr, cap))

    def set_instance_index_field(self, pool_id, offset):
        """gv_pool_set_instance_index_field: where a draw emission writes the uint32 index within the draw (None: nowhere)."""
        self._check(self.lib.gv_pool_set_instance_index_field(self.ctx, pool_id, GV_NONE if offset is None else int(offset)))

    def draw_bases_device(self, pool_id):
        """(device pointer of uint32 first_instance[draws + 1], device pointer of uint32 draw_starts[views + 1]) of the pool's last
        draw emission"""
        first, starts = C.c_void_p(), C.c_void_p()
        self._check(self.lib.gv_pool_draw_bases_device(self.ctx, pool_id, C.byref(first), C.byref(starts)))
        return first.value, starts.value

    def draw_bases(self, pool_id):
        """gv_pool_draw_bases_fetch: waits for the pool's last draw emission; returns (first_instance[draws + 1] — the first instance
        of every draw of the listed views, back to back, and the grand total behind them — and draw_starts[views + 1])."""
        views = self.instances_info(pool_id)[0]
        starts = np.zeros(views + 1, np.uint32)
        sp = starts.ctypes.data_as(C.POINTER(C.c_uint32))
        self._check(self.lib.gv_pool_draw_bases_fetch(self.ctx, pool_id, None, 0, sp, len(starts)))
        first = np.zeros(int(starts[views]) + 1, np.uint32)
        self._check(self.lib.gv_pool_draw_bases_fetch(self.ctx, pool_id, first.ctypes.data_as(C.POINTER(C.c_uint32)), len(first), sp, len(starts)))
        return first, starts

    def instances_info(self, pool_id):
        """(listed views, stride, instances the target holds) of the pool's last emission"""
        views, stride, capacity = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self.lib.gv_pool_instances_info(self.ctx, pool_id, C.byref(views), C.byref(stride), C.byref(capacity)))
        return views.value, stride.value, capacity.value

    def instances_device(self, pool_id):
        """(device pointer of the instances, device pointer of uint32 starts[views + 1]) of the pool's last emission"""
        inst, starts = C.c_void_p(), C.c_void_p()
        self._check(self.lib.gv_pool_instances_device(self.ctx, pool_id, C.byref(inst), C.byref(starts)))
        return inst.value, starts.value

    def instances(self, pool_id, out=None, dtype=None):
        """gv_pool_instances_fetch: waits for the pool's last emission; returns (instances [total, stride] as uint8 — or viewed as
        the structured `dtype` — and starts[views + 1]). out: the caller's own C-contiguous array to deliver into (only the layout's
        fields are written: its other bytes stay); default a zero-filled one."""
        views, stride, _ = self.instances_info(pool_id)
        starts = np.zeros(views + 1, np.uint32)
        sp = starts.ctypes.data_as(C.POINTER(C.c_uint32))
        self._check(self.lib.gv_pool_instances_fetch(self.ctx, pool_id, None, 0, sp, len(starts)))
        total = int(starts[views])
        if out is None:
            out = np.zeros((total, stride), np.uint8)
        assert out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]
        self._check(self.lib.gv_pool_instances_fetch(self.ctx, pool_id, out.ctypes.data, out.nbytes, sp, len(starts)))
        if dtype is not None:
            out = out.reshape(-1).view(np.uint8)[:total * stride].view(np.dtype(dtype))
        return out, starts

    # ---- indirect draw commands ----
    def bind_geometry(self, pool_id, ids, table):
        """gv_pool_bind_geometry: the pool's geometry ids (numpy u8 / u16 / u32 array, one element per slot, any element stride;
        None: every slot draws table[0]) and the geometry table (rows of (count, first, vertex_offset); copied at the call). Both
        None removes the binding. The caller keeps `ids` alive and unmoved, as for bind_ready."""
        if table is None:
            rows, tp, n = None, None, 0
        else:
            rows = np.asarray(table)
            if rows.dtype.names is None:  # plain rows of three numbers
                plain = rows.reshape(-1, 3)
                rows = np.zeros(len(plain), GEOMETRY_DTYPE)
                rows["count"], rows["first"], rows["vertex_offset"] = plain[:, 0], plain[:, 1], plain[:, 2]
            rows = np.ascontiguousarray(rows)
            assert rows.dtype.itemsize == C.sizeof(GvGeometry)
            tp, n = C.cast(rows.ctypes.data, C.POINTER(GvGeometry)), len(rows)
        if ids is None:
            self._keep.pop(("geometry", pool_id), None)
            self._check(self.lib.gv_pool_bind_geometry(self.ctx, pool_id, None, 0, 0, 0, tp, n))
            return
        assert ids.ndim == 1
        self._keep[("geometry", pool_id)] = ids
        self._check(self.lib.gv_pool_bind_geometry(self.ctx, pool_id, ids.ctypes.data, ids.strides[0], ids.dtype.itemsize, ids.shape[0], tp, n))

    def set_command_layout(self, pool_id, dtype=None, offsets=None):
        """gv_pool_set_command_layout: the caller's command struct, as a numpy structured `dtype` with the uint32 fields count,
        instance_count, first, first_instance and optionally vertex_offset (int32) and draw — or as `offsets`, a dict of the same
        names plus stride. Neither: the layout is removed."""
        if dtype is not None:
            dtype = np.dtype(dtype)
            offsets = {name: dtype.fields[name][1] for name in dtype.names}
            offsets["stride"] = dtype.itemsize
        if offsets is None:
            self._check(self.lib.gv_pool_set_command_layout(self.ctx, pool_id, None))
            return
        at = lambda name: GV_NONE if offsets.get(name) is None else int(offsets[name])
        layout = GvCommandLayout(int(offsets["stride"]), int(offsets["count"]), int(offsets["instance_count"]), int(offsets["first"]),
                                 int(offsets["first_instance"]), at("vertex_offset"), at("draw"))
        self._check(self.lib.gv_pool_set_command_layout(self.ctx, pool_id, C.byref(layout)))
        self._command_stride = getattr(self, "_command_stride", {})
        self._command_stride[pool_id] = layout.stride

    def emit_draw_commands(self, pool_id, merge_runs=False, region=0, device=None, flags=None):
        """gv_pool_emit_draw_commands: one indirect command per draw (merge_runs: per run of one geometry) of the pool's last
        instance emission, on the context's stream. region: 0 packs the views' commands, R > 0 gives every view R positions.
        device: None for the library's own buffer, or (device pointer, capacity in bytes) of caller-owned device memory."""
        ptr, cap = (None, 0) if device is None else (int(device[0]), int(device[1]))
        flags = (GV_COMMANDS_MERGE_RUNS if merge_runs else 0) if flags is None else flags
        self._check(self.lib.gv_pool_emit_draw_commands(self.ctx, pool_id, flags, int(region), ptr, cap))
        stride = self._command_stride[pool_id]
        self._commands = getattr(self, "_commands", {})
        self._commands[pool_id] = (stride, int(region), None if device is None else cap // stride)

    def draw_commands_device(self, pool_id):
        """(device pointer of the commands, device pointer of uint32 command_counts[views]) of the pool's last command emission"""
        commands, counts = C.c_void_p(), C.c_void_p()
        self._check(self.lib.gv_pool_draw_commands_device(self.ctx, pool_id, C.byref(commands), C.byref(counts)))
        return commands.value, counts.value

    def draw_commands(self, pool_id, dtype=None, out=None):
        """gv_pool_draw_commands_fetch: waits for the pool's last command emission; returns (the command positions — packed: the
        views' commands back to back; regions: views x region — as uint8 [positions, stride] or viewed as the structured `dtype`,
        and command_counts[views]). Positions a too small caller-owned device target does not hold stay as `out` has them
        (default zeros)."""
        stride, region, room = self._commands[pool_id]
        views = self.instances_info(pool_id)[0]
        counts = np.zeros(views, np.uint32)
        cp = counts.ctypes.data_as(C.POINTER(C.c_uint32))
        self._check(self.lib.gv_pool_draw_commands_fetch(self.ctx, pool_id, None, 0, cp, len(counts)))
        positions = views * region if region else int(counts.sum())
        if out is None:
            out = np.zeros((positions, stride), np.uint8)
        assert out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"] and out.nbytes >= (positions if room is None else min(positions, room)) * stride
        self._check(self.lib.gv_pool_draw_commands_fetch(self.ctx, pool_id, out.ctypes.data, out.nbytes, cp, len(counts)))
        if dtype is not None:
            out = out.reshape(-1).view(np.uint8)[:positions * stride].view(np.dtype(dtype))
        return out, counts

    # ---- mesh clusters, culled per draw ----
    def bind_clusters(self, pool_id, ranges, clusters):
        """gv_pool_bind_clusters: per geometry id a range (CLUSTER_RANGE_DTYPE, or rows of (first, count)) into the cluster table
        (CLUSTER_DTYPE: a model-space box, first index relative to the geometry's and index count). Both copied at the call; both
        None removes the binding."""
        if ranges is None and clusters is None:
            self._check(self.lib.gv_pool_bind_clusters(self.ctx, pool_id, None, 0, None, 0))
            return
        r = np.asarray(ranges)
        if r.dtype != CLUSTER_RANGE_DTYPE:  # plain rows of two numbers
            plain = r.reshape(-1, 2)
            r = np.zeros(len(plain), CLUSTER_RANGE_DTYPE)
            r["first"], r["count"] = plain[:, 0], plain[:, 1]
        r = np.ascontiguousarray(r)
        c = np.ascontiguousarray(clusters)
        assert c.dtype == CLUSTER_DTYPE and c.dtype.itemsize == C.sizeof(GvCluster) and r.dtype.itemsize == C.sizeof(GvClusterRange)
        self._check(self.lib.gv_pool_bind_clusters(self.ctx, pool_id, C.cast(r.ctypes.data, C.POINTER(GvClusterRange)), len(r),
                                                   C.cast(c.ctypes.data, C.POINTER(GvCluster)), len(c)))

    def bind_cluster_cones(self, pool_id, cones):
        """gv_pool_bind_cluster_cones: one normal cone (CLUSTER_CONE_DTYPE) per entry of the bound cluster table, copied at the call;
        None removes the binding."""
        if cones is None:
            self._check(self.lib.gv_pool_bind_cluster_cones(self.ctx, pool_id, None, 0))
            return
        c = np.ascontiguousarray(cones)
        assert c.dtype == CLUSTER_CONE_DTYPE and c.dtype.itemsize == 32
        self._check(self.lib.gv_pool_bind_cluster_cones(self.ctx, pool_id, c.ctypes.data, len(c)))

    def bind_cluster_lods(self, pool_id, lods):
        """gv_pool_bind_cluster_lods: one LOD entry (CLUSTER_LOD_DTYPE) per entry of the bound cluster table, copied at the call;
        None removes the binding."""
        if lods is None:
            self._check(self.lib.gv_pool_bind_cluster_lods(self.ctx, pool_id, None, 0))
            return
        t = np.ascontiguousarray(lods)
        assert t.dtype == CLUSTER_LOD_DTYPE and t.dtype.itemsize == 48
        self._check(self.lib.gv_pool_bind_cluster_lods(self.ctx, pool_id, t.ctypes.data, len(t)))

    def cull_clusters(self, pool_id, frustum_only=False, region=0, device=None, runs=False, eyes=None, lods=None):
        """gv_pool_cull_clusters: one indirect command per surviving cluster of every draw of the pool's last instance emission
        (draws without clusters are drawn whole), on the context's stream. frustum_only: no Hi-Z query even for views that named a
        pyramid. region: 0 packs the views' commands, R > 0 gives every view R positions. device: None for the library's own
        buffer, or (device pointer, capacity in bytes) of caller-owned device memory. runs: gv_pool_cull_cluster_runs — the same
        decisions, one command per run of adjacent surviving clusters (at most GV_CLUSTER_RUN_SPAN of them). eyes: an [m, 4]
        float32 array, one eye per view of the emission — gv_pool_cull_cluster_cones: a cluster whose bound normal cone faces away
        from its view's eye is rejected too (w != 0: a point eye, w == 0: parallel rays along xyz, all zero: no cone test); it
        combines with runs and frustum_only. lods: an array of CLUSTER_LOD_VIEW_DTYPE, one per view of the emission —
        gv_pool_cull_cluster_lods: only the clusters on the cut through the bound cluster DAG are drawn (their own error small enough
        on screen, their parent's not; scale 0: no LOD test for the view). Every cluster is still visited and counted as tested; a
        LOD-rejected one skips the plane tests, the cone test and the Hi-Z query. It combines with eyes, runs and frustum_only."""
        ptr, cap = (None, 0) if device is None else (int(device[0]), int(device[1]))
        if lods is not None:
            lv = np.ascontiguousarray(lods)
            assert lv.dtype == CLUSTER_LOD_VIEW_DTYPE and lv.dtype.itemsize == 32
            e = None if eyes is None else np.ascontiguousarray(eyes, np.float32).reshape(-1, 4)
            flags = (GV_CLUSTERS_FRUSTUM_ONLY if frustum_only else 0) | (GV_CLUSTERS_RUNS if runs else 0)
            self._check(self.lib.gv_pool_cull_cluster_lods(self.ctx, pool_id, flags, lv.ctypes.data, len(lv), None if e is None else e.ctypes.data,
                                                           0 if e is None else len(e), int(region), ptr, cap))
        elif eyes is not None:
            e = np.ascontiguousarray(eyes, np.float32).reshape(-1, 4)
            flags = (GV_CLUSTERS_FRUSTUM_ONLY if frustum_only else 0) | (GV_CLUSTERS_RUNS if runs else 0)
            self._check(self.lib.gv_pool_cull_cluster_cones(self.ctx, pool_id, flags, e.ctypes.data, len(e), int(region), ptr, cap))
        else:
            call = self.lib.gv_pool_cull_cluster_runs if runs else self.lib.gv_pool_cull_clusters
            self._check(call(self.ctx, pool_id, GV_CLUSTERS_FRUSTUM_ONLY if frustum_only else 0, int(region), ptr, cap))
        stride = self._command_stride[pool_id]
        self._cluster_commands = getattr(self, "_cluster_commands", {})
        self._cluster_commands[pool_id] = (stride, int(region), None if device is None else cap // stride)

    def cluster_commands_device(self, pool_id):
        """(device pointer of the commands, device pointer of uint32 counts[2 * views]) of the pool's last cluster cull"""
        commands, counts = C.c_void_p(), C.c_void_p()
        self._check(self.lib.gv_pool_cluster_commands_device(self.ctx, pool_id, C.byref(commands), C.byref(counts)))
        return commands.value, counts.value

    def cluster_commands(self, pool_id, dtype=None, out=None):
        """gv_pool_cluster_commands_fetch: waits for the pool's last cluster cull; returns (the command positions — packed: the
        views' commands back to back; regions: views x region — as uint8 [positions, stride] or viewed as the structured `dtype`,
        counts[views], tested[views]). Positions a too small caller-owned device target does not hold stay as `out` has them
        (default zeros)."""
        stride, region, room = self._cluster_commands[pool_id]
        views = self.instances_info(pool_id)[0]
        both = np.zeros(2 * views, np.uint32)
        cp = both.ctypes.data_as(C.POINTER(C.c_uint32))
        self._check(self.lib.gv_pool_cluster_commands_fetch(self.ctx, pool_id, None, 0, cp, len(both)))
        positions = views * region if region else int(both[:views].sum())
        if out is None:
            out = np.zeros((positions, stride), np.uint8)
        assert out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"] and out.nbytes >= (positions if room is None else min(positions, room)) * stride
        self._check(self.lib.gv_pool_cluster_commands_fetch(self.ctx, pool_id, out.ctypes.data, out.nbytes, cp, len(both)))
        if dtype is not None:
            out = out.reshape(-1).view(np.uint8)[:positions * stride].view(np.dtype(dtype))
        return out, both[:views].copy(), both[views:].copy()

    def cull_clusters_second_phase(self, pool_id, region=0, target=None):
        """gv_pool_cull_clusters_second_phase: the clusters the pool's last cull_clusters tested and did not keep, in the views for
        which it queried a pyramid, tested again against that pyramid as it stands now; one indirect command per survivor, in
        buffers of its own. region and target (None, or (device pointer, capacity in bytes)) as cull_clusters' region and device."""
        ptr, cap = (None, 0) if target is None else (int(target[0]), int(target[1]))
        self._check(self.lib.gv_pool_cull_clusters_second_phase(self.ctx, pool_id, 0, int(region), ptr, cap))
        stride = self._cluster_commands[pool_id][0]  # (the layout of the cluster cull it follows)
        self._cluster_second = getattr(self, "_cluster_second", {})
        self._cluster_second[pool_id] = (stride, int(region), None if target is None else cap // stride)

    def cluster_second_commands_device(self, pool_id):
        """(device pointer of the commands, device pointer of uint32 counts[2 * views]) of the pool's last cluster second phase"""
        commands, counts = C.c_void_p(), C.c_void_p()
        self._check(self.lib.gv_pool_cluster_second_commands_device(self.ctx, pool_id, C.byref(commands), C.byref(counts)))
        return commands.value, counts.value

    def cluster_second_commands(self, pool_id, dtype=None, out=None):
        """gv_pool_cluster_second_commands_fetch: as cluster_commands, of the pool's last cluster second phase; returns (the
        command positions, counts[views], pending[views] — the clusters re-tested per view)."""
        stride, region, room = self._cluster_second[pool_id]
        views = self.instances_info(pool_id)[0]
        both = np.zeros(2 * views, np.uint32)
        cp = both.ctypes.data_as(C.POINTER(C.c_uint32))
        self._check(self.lib.gv_pool_cluster_second_commands_fetch(self.ctx, pool_id, None, 0, cp, len(both)))
        positions = views * region if region else int(both[:views].sum())
        if out is None:
            out = np.zeros((positions, stride), np.uint8)
        assert out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"] and out.nbytes >= (positions if room is None else min(positions, room)) * stride
        self._check(self.lib.gv_pool_cluster_second_commands_fetch(self.ctx, pool_id, out.ctypes.data, out.nbytes, cp, len(both)))
        if dtype is not None:
            out = out.reshape(-1).view(np.uint8)[:positions * stride].view(np.dtype(dtype))
        return out, both[:views].copy(), both[views:].copy()

    # ---- level of detail per draw ----
    def bind_lod(self, pool_id, sizes, table):
        """gv_pool_bind_lod: the pool's sizes (numpy float32 array, one element per slot, any element stride; None: every slot has
        size 1) and the LOD table the BASE geometry ids index (a LOD_DTYPE array, or rows of (levels, [switch_at ...]); copied at
        the call). Both None removes the binding. The caller keeps `sizes` alive and unmoved, as for bind_ready."""
        if table is None:
            rows, tp, n = None, None, 0
        else:
            if isinstance(table, np.ndarray) and table.dtype == LOD_DTYPE:
                rows = np.ascontiguousarray(table)
            else:
                rows = np.zeros(len(table), LOD_DTYPE)
                for k, (levels, switch_at) in enumerate(table):
                    rows[k]["levels"] = levels
                    rows[k]["switch_at"][:len(switch_at)] = switch_at
            assert rows.dtype.itemsize == C.sizeof(GvLodGeometry)
            tp, n = C.cast(rows.ctypes.data, C.POINTER(GvLodGeometry)), len(rows)
        if sizes is None:
            self._keep.pop(("lod", pool_id), None)
            self._check(self.lib.gv_pool_bind_lod(self.ctx, pool_id, None, 0, 0, tp, n))
            return
        assert sizes.ndim == 1 and sizes.dtype == np.float32
        self._keep[("lod", pool_id)] = sizes
        self._check(self.lib.gv_pool_bind_lod(self.ctx, pool_id, sizes.ctypes.data, sizes.strides[0], sizes.shape[0], tp, n))

    def select_lods(self, pool_id, view_scale):
        """gv_pool_select_lods: the level of detail of every draw of the pool's last instance emission, on the context's stream;
        view_scale: one float per listed view. None drops the selection. A command emission that follows takes the selected ids."""
        if view_scale is None:
            self._check(self.lib.gv_pool_select_lods(self.ctx, pool_id, None, 0))
            return
        scale = np.ascontiguousarray(view_scale, dtype=np.float32).reshape(-1)
        self._check(self.lib.gv_pool_select_lods(self.ctx, pool_id, scale.ctypes.data_as(C.POINTER(C.c_float)), len(scale)))

    def lods_device(self, pool_id):
        """(device pointer of uint32 draw_geometry[draws], device pointer of uint32 level_counts[views * 8]) of the pool's selection"""
        ids, counts = C.c_void_p(), C.c_void_p()
        self._check(self.lib.gv_pool_lods_device(self.ctx, pool_id, C.byref(ids), C.byref(counts)))
        return ids.value, counts.value

    def lods(self, pool_id):
        """gv_pool_lods_fetch: waits for the pool's selection; returns (the selected geometry ids g_k as one uint32 array per listed
        view, level_counts as uint32 [views, 8])."""
        views = self.instances_info(pool_id)[0]
        counts = np.zeros(views * GV_MAX_LOD_LEVELS, np.uint32)
        cp = counts.ctypes.data_as(C.POINTER(C.c_uint32))
        self._check(self.lib.gv_pool_lods_fetch(self.ctx, pool_id, None, 0, cp, len(counts)))
        ids = np.zeros(max(int(counts.sum()), 1), np.uint32)
        self._check(self.lib.gv_pool_lods_fetch(self.ctx, pool_id, ids.ctypes.data_as(C.POINTER(C.c_uint32)), len(ids), cp, len(counts)))
        counts = counts.reshape(views, GV_MAX_LOD_LEVELS)
        ends = np.cumsum(counts.sum(axis=1, dtype=np.int64))
        return [ids[int(e - c):int(e)].copy() for e, c in zip(ends, counts.sum(axis=1, dtype=np.int64))], counts

    # ---- the shared sorted arrays ----
    @staticmethod
    def merge_groups(groups):
        """The GvMergeGroup array of `groups`: dicts with group_id, items — (pool_id, view_index, buffer_index, component_stride)
        each —, descending, dtype (a numpy structured record type with componentOffset, bakedModel, distanceSq and optionally
        bufferIndex; or the keys stride / component_offset / baked_model / distance_sq / buffer_index) and optionally device =
        (device pointer, capacity in bytes). Returns (array, the item arrays it points into)."""
        arr, keep = (GvMergeGroup * max(len(groups), 1))(), []
        for g, d in zip(arr, groups):
            items = (GvMergeItem * max(len(d["items"]), 1))(*[GvMergeItem(*[int(x) for x in it]) for it in d["items"]])
            keep.append(items)
            g.group_id, g.item_count, g.items, g.descending = int(d["group_id"]), len(d["items"]), items, 1 if d.get("descending") else 0
            if d.get("dtype") is not None:
                dtype = np.dtype(d["dtype"])
                at = {name: dtype.fields[name][1] for name in dtype.names}
                g.stride, g.component_offset, g.baked_model, g.distance_sq = dtype.itemsize, at["componentOffset"], at["bakedModel"], at["distanceSq"]
                g.buffer_index = at.get("bufferIndex", GV_NONE)
            else:
                g.stride, g.component_offset, g.baked_model, g.distance_sq = (int(d[k]) for k in ("stride", "component_offset", "baked_model", "distance_sq"))
                g.buffer_index = GV_NONE if d.get("buffer_index") is None else int(d["buffer_index"])
            if d.get("device") is not None:
                g.dst_device, g.capacity_bytes = int(d["device"][0]), int(d["device"][1])
        return arr, keep

    def merge_sorted(self, groups):
        """gv_merge_sorted: the sorted lists of each group's (pool, view) members merged into one record array per group, all groups
        by one launch on the context's stream (groups: see merge_groups)."""
        arr, keep = self.merge_groups(groups)
        self._check(self.lib.gv_merge_sorted(self.ctx, arr, len(groups)))
        del keep
        if not hasattr(self, "_merge_items"):
            self._merge_items = {}
        for d in groups:
            self._merge_items[int(d["group_id"])] = len(d["items"])

    def merge_device(self, group_id):
        """(device pointer of the merged records, device pointer of uint32 counts[items + 1]) of the group's last merge"""
        rec, counts = C.c_void_p(), C.c_void_p()
        self._check(self.lib.gv_merge_device(self.ctx, group_id, C.byref(rec), C.byref(counts)))
        return rec.value, counts.value

    def merged(self, group_id, dtype):
        """gv_merge_fetch: waits for the group's merge; returns (the records [0, total) viewed as the structured `dtype`, and
        counts[items + 1]: every member's draw count, then the total)."""
        dtype = np.dtype(dtype)
        counts = np.zeros(GV_MAX_MERGE_ITEMS + 1, np.uint32)
        cp = counts.ctypes.data_as(C.POINTER(C.c_uint32))
        self._check(self.lib.gv_merge_fetch(self.ctx, group_id, None, 0, cp, len(counts)))
        item_count = getattr(self, "_merge_items", {}).get(group_id, 0)
        total = int(counts[item_count])
        out = np.zeros(total * dtype.itemsize, np.uint8)
        self._check(self.lib.gv_merge_fetch(self.ctx, group_id, out.ctypes.data, out.nbytes, cp, len(counts)))
        return out.view(dtype), counts[:item_count + 1].copy()

    # ---- world matrices ----
    def sweep(self, mode=GV_SWEEP_VALU):
        self._check(self.lib.gv_sweep(self.ctx, mode))

    def get_world(self, first, count):
        out = np.empty((count, 12), dtype=np.float32)
        self._check(self.lib.gv_get_world(self.ctx, first, count, out.ctypes.data))
        return out

    # ---- Hi-Z ----
    def hiz_build(self, depth, mem_kind=GV_MEM_HOST):
        """mem_kind=GV_MEM_DEVICE: `depth` is a contiguous fp32 [height, width] tensor on this context's device (anything with
        data_ptr(), shape and is_contiguous(), e.g. a torch tensor). It is not copied: the pyramid, hiz_rebuild and the queries
        read it where it is, so the caller keeps it alive and orders its own writes to it against the library's stream."""
        if mem_kind == GV_MEM_DEVICE:
            height, width = depth.shape
            if not depth.is_contiguous() or depth.element_size() != 4 or not depth.is_floating_point():
                raise ValueError("hiz_build(GV_MEM_DEVICE): a contiguous fp32 [height, width] device tensor is required")
            self._check(self.lib.gv_hiz_build(self.ctx, depth.data_ptr(), width, height, GV_MEM_DEVICE))
            return
        d = np.ascontiguousarray(depth, dtype=np.float32)
        self._check(self.lib.gv_hiz_build(self.ctx, d.ctypes.data, d.shape[1], d.shape[0], GV_MEM_HOST))

    def hiz_rebuild(self):
        self._check(self.lib.gv_hiz_rebuild(self.ctx))

    def hiz_select(self, pyramid):
        """gv_hiz_select: pyramid `pyramid` (0 .. GV_MAX_PYRAMIDS - 1) is the one hiz_build, hiz_rebuild, hiz_read_level, hiz_mip_count
        and the two hiz_build_from_* address from here on. A view names the pyramid it queries itself: make_view(use_hiz=1 + k)."""
        self._check(self.lib.gv_hiz_select(self.ctx, pyramid))

    def hiz_drop(self, pyramid):
        """gv_hiz_drop: frees that pyramid's levels (an image it was built from stays); it is not built afterwards"""
        self._check(self.lib.gv_hiz_drop(self.ctx, pyramid))

    # ---- occluder depth ----
    def bind_occluders(self, pool_id, box_min, box_max):
        """gv_pool_bind_occluders: per-slot occluder boxes in model space (fp32 [n, 3+] each, C-contiguous rows of one common row
        stride; None, None removes the binding). The caller keeps them alive and unmoved; edits are reported with GV_DIRTY_OCCLUDER.
        The binder's contract: a box lies inside what the slot draws — the library does not check it."""
        if box_min is None and box_max is None:
            self._keep.pop(("occluders", pool_id), None)
            self._check(self.lib.gv_pool_bind_occluders(self.ctx, pool_id, None, None, 0, 0))
            return
        if box_min.dtype != np.float32 or box_max.dtype != np.float32 or box_min.ndim != 2 or box_min.shape[0] != box_max.shape[0] \
                or box_min.strides != box_max.strides or box_min.strides[1] != 4 or box_min.shape[1] < 3 or box_max.shape[1] < 3:
            raise ValueError("bind_occluders: two fp32 [n, 3+] arrays of the same row stride")
        self._keep[("occluders", pool_id)] = (box_min, box_max)
        self._check(self.lib.gv_pool_bind_occluders(self.ctx, pool_id, box_min.ctypes.data, box_max.ctypes.data, box_min.strides[0],
                                                    box_min.shape[0]))

    def occluder_begin(self, width, height):
        """gv_occluder_begin: opens (sizes, clears) the occluder image the current pyramid does not read; asynchronous"""
        self._check(self.lib.gv_occluder_begin(self.ctx, width, height))

    def draw_occluders(self, pool_id, view_index, min_pixels=1):
        """gv_pool_draw_occluders: the occluder boxes of the view's draws into the open image; asynchronous"""
        self._check(self.lib.gv_pool_draw_occluders(self.ctx, pool_id, view_index, min_pixels))

    def occluder_depth_device(self):
        """gv_occluder_depth_device: (device pointer of the image, width, height, device pointer of the six counts)"""
        depth, counts, w, h = C.c_void_p(), C.c_void_p(), C.c_uint32(), C.c_uint32()
        self._check(self.lib.gv_occluder_depth_device(self.ctx, C.byref(depth), C.byref(w), C.byref(h), C.byref(counts)))
        return depth.value, w.value, h.value, counts.value

    def occluder_depth(self):
        """gv_occluder_depth_fetch: waits; (image fp32 [height, width], counts as a dict of the six fields)"""
        _, w, h, _ = self.occluder_depth_device()
        image = np.empty((h, w), np.float32)
        counts = GvOccluderCounts()
        self._check(self.lib.gv_occluder_depth_fetch(self.ctx, image.ctypes.data, image.nbytes, C.byref(counts)))
        return image, {name: int(getattr(counts, name)) for name in OCCLUDER_COUNT_NAMES}

    def hiz_build_from_occluders(self):
        """gv_hiz_build_from_occluders: the pyramid of the open image (not copied), which it closes"""
        self._check(self.lib.gv_hiz_build_from_occluders(self.ctx))

    # ---- receiver mask ----
    def receiver_begin(self, width, height):
        """gv_receiver_begin: opens (sizes, clears to +inf) the receiver image the current pyramid does not read; asynchronous"""
        self._check(self.lib.gv_receiver_begin(self.ctx, width, height))

    def draw_receivers(self, pool_id, view_index, light_view_proj):
        """gv_pool_draw_receivers: the cull AABBs of the view's draws into the open mask, projected with light_view_proj (16 fp32,
        column-major; copied by the call); asynchronous"""
        light = np.ascontiguousarray(light_view_proj, dtype=np.float32).reshape(16)
        self._check(self.lib.gv_pool_draw_receivers(self.ctx, pool_id, view_index, light.ctypes.data))

    def receiver_mask_device(self):
        """gv_receiver_mask_device: (device pointer of the mask, width, height, device pointer of the counts)"""
        mask, counts, w, h = C.c_void_p(), C.c_void_p(), C.c_uint32(), C.c_uint32()
        self._check(self.lib.gv_receiver_mask_device(self.ctx, C.byref(mask), C.byref(w), C.byref(h), C.byref(counts)))
        return mask.value, w.value, h.value, counts.value

    def receiver_mask(self):
        """gv_receiver_mask_fetch: waits; (mask fp32 [height, width], counts as a dict of the six fields)"""
        _, w, h, _ = self.receiver_mask_device()
        image = np.empty((h, w), np.float32)
        counts = GvReceiverCounts()
        self._check(self.lib.gv_receiver_mask_fetch(self.ctx, image.ctypes.data, image.nbytes, C.byref(counts)))
        return image, {name: int(getattr(counts, name)) for name in RECEIVER_COUNT_NAMES}

    def hiz_build_from_receivers(self):
        """gv_hiz_build_from_receivers: the pyramid of the open mask (not copied), which it closes"""
        self._check(self.lib.gv_hiz_build_from_receivers(self.ctx))

    # ---- last frame's mvp per draw (motion vectors) ----
    def keep_models(self, pool_id, view_index=0, add=False):
        """gv_pool_keep_models: the models the view delivered become the pool's history, by pool slot (add: GV_KEEP_ADD, the second
        view of a two-phase frame joins the epoch of the first); asynchronous, call it behind emit_previous"""
        self._check(self.lib.gv_pool_keep_models(self.ctx, pool_id, view_index, GV_KEEP_ADD if add else 0))

    def forget_models(self, pool_id, first=0, count=0):
        """gv_pool_forget_models: slots [first, first + count) are fresh at the next emission; count 0 empties the whole history"""
        self._check(self.lib.gv_pool_forget_models(self.ctx, pool_id, first, count))

    def emit_previous(self, pool_id, view_index=0, stride=64, prev_mvp=0, has_history=None, prev_view_proj=None, cut=False, device=None,
                      layout=True):
        """gv_pool_emit_previous: last frame's viewProj * model of every draw of the view (and whether the draw had a history), on the
        context's stream. layout=False passes a NULL layout ({64, 0, none}); prev_view_proj None: the kept view's; device: None for
        the library's own buffer, or (device pointer, capacity in bytes) of caller-owned device memory."""
        L = GvPreviousLayout(int(stride), int(prev_mvp), GV_NONE if has_history is None else int(has_history))
        pvp = None
        if prev_view_proj is not None:
            held = np.ascontiguousarray(prev_view_proj, dtype=np.float32).reshape(16)
            pvp = held.ctypes.data_as(C.POINTER(C.c_float))
        ptr, cap = (None, 0) if device is None else (int(device[0]), int(device[1]))
        self._check(self.lib.gv_pool_emit_previous(self.ctx, pool_id, view_index, C.byref(L) if layout else None, pvp,
                                                   GV_PREVIOUS_CUT if cut else 0, ptr, cap))
        self._previous_stride = int(stride) if layout else 64

    def previous_device(self, pool_id):
        """gv_pool_previous_device: (device pointer of the items, device pointer of the four counts) of the pool's last emission"""
        items, counts = C.c_void_p(), C.c_void_p()
        self._check(self.lib.gv_pool_previous_device(self.ctx, pool_id, C.byref(items), C.byref(counts)))
        return items.value, counts.value

    def previous(self, pool_id, out=None, stride=None, counts_only=False):
        """gv_pool_previous_fetch: waits for the pool's last emit_previous; returns (items [written, stride] as uint8, counts = {n,
        kept draws, items written, e} as four uint32). out: the caller's own C-contiguous array to deliver into (only the layout's
        fields are written: its other bytes stay); default a zero-filled one. stride: default that of this object's last emit_previous.
        counts_only: waits and returns (None, counts)."""
        stride = int(stride if stride is not None else getattr(self, "_previous_stride", 64))
        counts = np.zeros(4, np.uint32)
        cp = counts.ctypes.data_as(C.POINTER(C.c_uint32))
        self._check(self.lib.gv_pool_previous_fetch(self.ctx, pool_id, None, 0, cp))
        if counts_only:
            return None, counts
        if out is None:
            out = np.zeros((int(counts[2]), stride), np.uint8)
        assert out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]
        self._check(self.lib.gv_pool_previous_fetch(self.ctx, pool_id, out.ctypes.data, out.nbytes, cp))
        return out, counts

    def hiz_mip_count(self):
        n = C.c_uint32()
        self._check(self.lib.gv_hiz_mip_count(self.ctx, C.byref(n)))
        return n.value

    def hiz_read_level(self, level, w, h):
        out = np.empty((h, w, 2), dtype=np.float32)
        rw, rh = C.c_uint32(), C.c_uint32()
        self._check(self.lib.gv_hiz_read_level(self.ctx, level, out.ctypes.data, C.byref(rw), C.byref(rh)))
        assert (rw.value, rh.value) == (w, h), (rw.value, rh.value, w, h)
        return out

    # ---- metrics ----
    def stats(self):
        s = GvStats()
        self._check(self.lib.gv_stats(self.ctx, C.byref(s)))
        return dict(launches={k: int(s.launches[i]) for i, k in enumerate(KERNEL_NAMES)},
                    device_ms={k: float(s.device_ms[i]) for i, k in enumerate(KERNEL_NAMES)},
                    upload_bytes=int(s.upload_bytes), mirror_reorders=int(s.mirror_reorders), record_targets_lost=int(s.record_targets_lost),
                    max_depth=int(s.max_depth),
                    transform_count=int(s.transform_count), bounds_blocks_total=int(s.bounds_blocks_total),
                    bounds_blocks_examined=int(s.bounds_blocks_examined))

    def stream_peak(self, pool_id=0, launches=20):
        """GB/s of a read-only pass over the cull kernel's input streams of `pool_id` (median of `launches`)."""
        g = C.c_double()
        self._check(self.lib.gv_debug_stream_peak(self.ctx, pool_id, launches, C.byref(g)))
        return g.value

    def stats_reset(self):
        self._check(self.lib.gv_stats_reset(self.ctx))

    def profile_sampling(self, every):
        """Bracket only every `every`-th launch of each kernel kind with events (each bracket costs ~5 us of stream time)."""
        self._check(self.lib.gv_profile_sampling(self.ctx, every))

    def profile_kernels(self, names):
        """Bracket the launches of these kernel kinds (KERNEL_NAMES) from now on; [] = none."""
        self._check(self.lib.gv_profile_kernels(self.ctx, sum(1 << KERNEL_NAMES.index(n) for n in names)))

    def profile_samples(self):
        """Bracketed launches per kernel kind since stats_reset: the divisor for stats()['device_ms']."""
        a = (C.c_uint64 * GV_K_COUNT)()
        self._check(self.lib.gv_profile_samples(self.ctx, C.byref(a)))
        return {k: int(a[i]) for i, k in enumerate(KERNEL_NAMES)}


def cell_owner(grid, side, world, positions):
    """Rank that owns each position (float32 [n, >= 3]) under the dealing rule of gv_scene_extract_rank (gv_cell_owner)."""
    pos = np.ascontiguousarray(positions, dtype=np.float32)
    out = np.empty(pos.shape[0], dtype=np.uint32)
    g = (C.c_uint32 * 3)(*[int(x) for x in grid])
    rc = load().gv_cell_owner(C.byref(g), float(side), int(world), pos.ctypes.data, pos.strides[0], pos.shape[0], out.ctypes.data)
    if rc != GV_OK:
        raise GvError(rc, "gv_cell_owner: bad argument")
    return out


class Scene:
    """A Garden scene file ingested straight into column pools (gv_scene_*; no device needed until bind)."""

    def __init__(self, text, pools, add_root_entity=False, bson=False):
        """text: the scene JSON (str or bytes), or with bson=True the BSON document packed builds ship (json2bson);
        pools: {component ".type": pool id}; add_root_entity: loadScene's addRootEntity (a default transform as
        entity 1, parent of everything that names no other parent)."""
        self.lib = load()
        raw = text.encode() if isinstance(text, str) else bytes(text)
        arr = (GvScenePool * max(len(pools), 1))(*[GvScenePool(k.encode(), v) for k, v in pools.items()])
        handle, err = C.c_void_p(), C.create_string_buffer(512)
        parse = self.lib.gv_scene_parse_bson if bson else self.lib.gv_scene_parse_json
        rc = parse(raw, len(raw), arr, len(pools), 1 if add_root_entity else 0, C.byref(handle), err, len(err))
        if rc != 0:
            raise GvError(rc, err.value.decode(errors="replace"))
        self.handle, self.pools = handle, dict(pools)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.gv_scene_destroy(self.handle)
            self.handle = None

    __del__ = close

    def info(self):
        i = GvSceneInfo()
        self.lib.gv_scene_info(self.handle, C.byref(i))
        out = {n: getattr(i, n) for n, _ in GvSceneInfo._fields_ if n != "mesh_count"}
        out["mesh_count"] = {pid: i.mesh_count[pid] for pid in self.pools.values()}
        return out

    @staticmethod
    def _view(col, n, dtype, width):
        if n == 0:
            return np.zeros((0, width) if width > 1 else 0, dtype)
        a = np.ctypeslib.as_array(C.cast(col.data, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(n * width,))
        return a.reshape(n, width).copy() if width > 1 else a.copy()

    def transform_columns(self):
        """Copies of the transform columns + entity_to_transform + uids, as numpy arrays."""
        c, n, cap, e2t, uids = GvTransformColumns(), C.c_uint32(), C.c_uint32(), C.c_void_p(), C.c_void_p()
        self.lib.gv_scene_transform_columns(self.handle, C.byref(c), C.byref(n), C.byref(e2t), C.byref(cap), C.byref(uids))
        n = n.value
        out = dict(entity=self._view(c.entity, n, np.uint32, 1), parent=self._view(c.parent, n, np.uint32, 1),
                   position=self._view(c.position, n, np.float32, 3), scale=self._view(c.scale, n, np.float32, 3),
                   rotation=self._view(c.rotation, n, np.float32, 4), self_active=self._view(c.self_active, n, np.uint8, 1),
                   ancestors_active=self._view(c.ancestors_active, n, np.uint8, 1),
                   model_with_ancestors=self._view(c.model_with_ancestors, n, np.uint8, 1))
        out["entity_to_transform"] = self._view(GvColumn(e2t.value, 4), cap.value, np.uint32, 1)
        out["uid"] = self._view(GvColumn(uids.value, 8), n, np.uint64, 1)
        return out

    def mesh_columns(self, pool_id):
        c, n = GvMeshColumns(), C.c_uint32()
        self.lib.gv_scene_mesh_columns(self.handle, pool_id, C.byref(c), C.byref(n))
        n = n.value
        return dict(entity=self._view(c.entity, n, np.uint32, 1), is_enabled=self._view(c.is_enabled, n, np.uint8, 1),
                    aabb_min=self._view(c.aabb_min, n, np.float32, 3), aabb_max=self._view(c.aabb_max, n, np.float32, 3),
                    is_visible=self._view(GvColumn(c.is_visible, 1), n, np.uint8, 1))

    def extract_tile(self, grid, side, tile):
        """One spatial tile of this scene as a Scene of its own (gv_scene_extract_tile)."""
        handle = C.c_void_p()
        g = (C.c_uint32 * 3)(*[int(x) for x in grid])
        rc = self.lib.gv_scene_extract_tile(self.handle, C.byref(g), float(side), int(tile), C.byref(handle))
        if rc != 0:
            raise GvError(rc, "gv_scene_extract_tile failed")
        t = Scene.__new__(Scene)
        t.lib, t.handle, t.pools = self.lib, handle, dict(self.pools)
        return t

    def extract_rank(self, grid, side, rank, world):
        """Everything rank `rank` of `world` owns (the grid's cells in Morton order, dealt round-robin) as one Scene
        (gv_scene_extract_rank; multi.py::cell_owners is the same table)."""
        handle = C.c_void_p()
        g = (C.c_uint32 * 3)(*[int(x) for x in grid])
        rc = self.lib.gv_scene_extract_rank(self.handle, C.byref(g), float(side), int(rank), int(world), C.byref(handle))
        if rc != 0:
            raise GvError(rc, "gv_scene_extract_rank failed")
        t = Scene.__new__(Scene)
        t.lib, t.handle, t.pools = self.lib, handle, dict(self.pools)
        return t

    def tile_maps(self, pool_id):
        """(transform_global, mesh_global) of a tile: local slot -> slot in the scene it was cut from."""
        tg, tn, mg, mn = C.c_void_p(), C.c_uint32(), C.c_void_p(), C.c_uint32()
        rc = self.lib.gv_scene_tile_maps(self.handle, pool_id, C.byref(tg), C.byref(tn), C.byref(mg), C.byref(mn))
        if rc != 0:
            raise GvError(rc, "gv_scene_tile_maps: not a tile")
        return (self._view(GvColumn(tg.value, 4), tn.value, np.uint32, 1), self._view(GvColumn(mg.value, 4), mn.value, np.uint32, 1))

    def bind(self, vis):
        """Binds the scene's columns to a GpuVisibility context (the scene must stay alive while bound)."""
        vis._scene = self
        vis._check(self.lib.gv_scene_bind(vis.ctx, self.handle))
