"""ctypes binding of libnbk.so (include/nbk.h).

The product path has NO CPU fallback: if the library is missing, or no GPU is visible when a compute
entry point is called, this module raises.  (Loading the library and reading its symbols works without
a GPU, which is what the CPU-side tests check.)
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libnbk.so")

NBK_OK = 0
# status codes of nbk_edge_continuous_batch / nbk_spline_continuous_batch (NBK_CA_*)
CA_FREE, CA_COLLISION, CA_UNDECIDED, CA_DEGENERATE = 0, 1, 2, 3
STATUS = {0: "NBK_OK", -1: "NBK_ERR_INVALID", -2: "NBK_ERR_NO_DEVICE", -3: "NBK_ERR_HIP",
          -4: "NBK_ERR_UNSUPPORTED", -5: "NBK_ERR_ALLOC"}

# every symbol include/nbk.h declares
SYMBOLS = [
    "nbk_abi_version", "nbk_status_string", "nbk_last_error", "nbk_device_count",
    "nbk_model_create", "nbk_model_destroy", "nbk_model_num_pairs",
    "nbk_fk_batch", "nbk_frameset_create", "nbk_frameset_destroy", "nbk_fk_frames_batch", "nbk_jacobian_batch", "nbk_ik_batch", "nbk_validity_batch", "nbk_validity_workspace_bytes",
    "nbk_validity_batch_ws", "nbk_closest_batch",
    "nbk_pair_distances_batch", "nbk_proximity_jacobian_batch", "nbk_pair_records_items", "nbk_edge_validity_batch",
    "nbk_edge_continuous_batch", "nbk_edge_motion_bounds_host", "nbk_selftest_math",
    "nbk_fk_batch_host", "nbk_validity_batch_host", "nbk_knn_prefix",
    "nbk_validity_scalar_host", "nbk_edge_validity_scalar_host", "nbk_spline_validity_batch",
    "nbk_spline_continuous_batch", "nbk_spline_motion_bounds_host",
    "nbk_broad_kernel_used", "nbk_broad_spec_source", "nbk_broad_spec_source_movable", "nbk_jit_compile",
    "nbk_model_create_movable", "nbk_model_set_world_poses", "nbk_model_set_world_poses_host", "nbk_model_world_status",
    "nbk_world_reach_bounds_host",
    "nbk_cloud_create", "nbk_cloud_destroy", "nbk_cloud_set_points", "nbk_cloud_status", "nbk_cloud_validity_batch",
    "nbk_cloud_clearance_batch", "nbk_cloud_cells_host", "nbk_records_cloud_batch",
    "nbk_edge_cloud_workspace_bytes", "nbk_edge_cloud_validity_batch",
    "nbk_edge_cloud_continuous_batch", "nbk_edge_shape_motion_bounds_host",
    "nbk_spline_cloud_workspace_bytes", "nbk_spline_cloud_validity_batch",
    "nbk_spline_cloud_continuous_batch", "nbk_spline_shape_motion_bounds_host",
    "nbk_frame_cloud_backproject", "nbk_frame_cloud_backproject_host", "nbk_frame_cloud_self_filter", "nbk_frame_cloud_self_filter_lds_bytes",
    "nbk_frame_cloud_set_points", "nbk_frame_cloud_count",
    "nbk_frame_cloud_carve", "nbk_frame_cloud_carve_host", "nbk_frame_cloud_novel", "nbk_frame_cloud_append_workspace_bytes",
    "nbk_frame_cloud_append",
    "nbk_render_depth_lds_bytes", "nbk_render_ray_spans_host", "nbk_render_depth_batch",
    "nbk_held_locals_host", "nbk_held_create", "nbk_held_destroy", "nbk_held_validity_batch",
    "nbk_edge_held_workspace_bytes", "nbk_edge_held_validity_batch",
    "nbk_held_item_count", "nbk_held_items", "nbk_held_distances_batch", "nbk_held_records_batch", "nbk_held_records_items",
    "nbk_edge_held_continuous_batch", "nbk_spline_held_continuous_batch",
    "nbk_spline_held_workspace_bytes", "nbk_spline_held_validity_batch",
    "nbk_edge_held_motion_bounds_host", "nbk_spline_held_motion_bounds_host",
    "nbk_held_create_hulls", "nbk_edge_held_motion_bounds_hulls_host", "nbk_spline_held_motion_bounds_hulls_host",
    "nbk_held_cloud_validity_batch", "nbk_held_cloud_clearance_batch", "nbk_held_cloud_records_batch",
    "nbk_edge_held_cloud_workspace_bytes", "nbk_edge_held_cloud_validity_batch",
    "nbk_spline_held_cloud_workspace_bytes", "nbk_spline_held_cloud_validity_batch",
    "nbk_edge_held_cloud_continuous_batch", "nbk_spline_held_cloud_continuous_batch",
    "nbk_edge_held_shape_motion_bounds_host", "nbk_spline_held_shape_motion_bounds_host",
    "nbk_held_set_cloud_hulls", "nbk_edge_held_shape_motion_bounds_hulls_host", "nbk_spline_held_shape_motion_bounds_hulls_host",
]
MAX_SPLINE_DEGREE = 5       # NBK_MAX_SPLINE_DEGREE


class ModelDesc(C.Structure):
    _fields_ = [
        ("n_q", C.c_int32), ("n_joints", C.c_int32),
        ("joint_parent", C.c_void_p), ("joint_type", C.c_void_p), ("joint_qidx", C.c_void_p),
        ("joint_rot", C.c_void_p), ("joint_trans", C.c_void_p), ("joint_slide", C.c_void_p),
        ("joint_axis", C.c_void_p), ("base_pose", C.c_void_p),
        ("n_rshapes", C.c_int32),
        ("rshape_frame", C.c_void_p), ("rshape_type", C.c_void_p), ("rshape_local", C.c_void_p),
        ("rshape_param", C.c_void_p),
        ("n_wshapes", C.c_int32),
        ("wshape_type", C.c_void_p), ("wshape_pose", C.c_void_p), ("wshape_param", C.c_void_p),
        ("n_pairs", C.c_int32),
        ("pair_a", C.c_void_p), ("pair_b", C.c_void_p),
        ("n_hulls", C.c_int32),
        ("hull_vert_begin", C.c_void_p), ("hull_verts", C.c_void_p),
        ("hull_face_begin", C.c_void_p), ("hull_planes", C.c_void_p),
    ]


class NbkError(RuntimeError):
    pass


_lib = None


def load():
    """Load libnbk.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NbkError(
            f"{LIB_PATH} is missing: build it with `python -m numbotics_amd.csrc.build` "
            "(or __graft_entry__.build()).  There is no CPU fallback for the device path.")
    # PyTorch-ROCm ships its own HIP runtime: load it first so that libnbk.so binds to the runtime torch uses (loaded the other
    # way round the process ends up with two runtimes and torch sees no device)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    lib.nbk_status_string.restype = C.c_char_p
    lib.nbk_status_string.argtypes = [C.c_int32]
    lib.nbk_last_error.restype = C.c_char_p
    lib.nbk_model_destroy.restype = None
    lib.nbk_model_destroy.argtypes = [C.c_void_p]
    lib.nbk_model_create.argtypes = [C.POINTER(ModelDesc), C.POINTER(C.c_void_p)]
    lib.nbk_model_create_movable.argtypes = [C.POINTER(ModelDesc), C.c_double, C.POINTER(C.c_void_p)]
    lib.nbk_model_set_world_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.nbk_model_set_world_poses_host.argtypes = [C.c_void_p, C.c_void_p]
    lib.nbk_model_world_status.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.nbk_world_reach_bounds_host.argtypes = [C.POINTER(ModelDesc), C.c_void_p, C.c_void_p]
    vp, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    lib.nbk_fk_batch.argtypes = [vp, vp, i64, vp, i32, vp, vp, vp, vp]
    lib.nbk_jacobian_batch.argtypes = [vp, vp, i64, vp, i32, vp, i32, vp, vp, vp]
    lib.nbk_frameset_create.argtypes = [vp, i32, vp, vp, vp]
    lib.nbk_frameset_destroy.argtypes = [vp]
    lib.nbk_frameset_destroy.restype = None
    lib.nbk_fk_frames_batch.argtypes = [vp, vp, vp, i64, vp, vp]
    lib.nbk_ik_batch.argtypes = [vp, vp, vp, i64, vp, i32, vp, vp, f64, i32, i32, vp, vp, vp, vp, vp]
    lib.nbk_validity_batch.argtypes = [vp, vp, i64, f64, vp, vp, vp]
    lib.nbk_broad_kernel_used.argtypes = [vp]
    lib.nbk_broad_spec_source.argtypes = [vp, C.c_char_p, i64]
    lib.nbk_broad_spec_source.restype = i64
    lib.nbk_jit_compile.argtypes = [C.c_char_p, C.c_char_p]
    lib.nbk_jit_compile.restype = i64
    lib.nbk_validity_workspace_bytes.argtypes = [vp, i64]
    lib.nbk_validity_workspace_bytes.restype = i64
    lib.nbk_validity_batch_ws.argtypes = [vp, vp, i64, f64, vp, vp, vp, i64, vp]
    lib.nbk_closest_batch.argtypes = [vp, vp, i64, vp, vp, vp]
    lib.nbk_pair_distances_batch.argtypes = [vp, vp, i64, vp, vp, vp]
    lib.nbk_proximity_jacobian_batch.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    lib.nbk_pair_records_items.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp]
    lib.nbk_edge_validity_batch.argtypes = [vp, vp, vp, vp, i64, f64, f64, i32, f64, vp, vp, vp, vp]
    lib.nbk_edge_continuous_batch.argtypes = [vp, vp, vp, vp, i64, f64, i32, f64, i32, f64, vp, vp, vp, vp, vp]
    lib.nbk_spline_validity_batch.argtypes = [vp, vp, i64, i32, i32, vp, f64, f64, vp, vp, vp, vp]
    lib.nbk_edge_motion_bounds_host.argtypes = [C.POINTER(ModelDesc), vp, vp, i64, vp]
    lib.nbk_spline_continuous_batch.argtypes = [vp, vp, i64, i32, i32, vp, f64, i32, f64, vp, vp, vp, vp]
    lib.nbk_spline_motion_bounds_host.argtypes = [C.POINTER(ModelDesc), vp, i64, i32, i32, vp, vp]
    lib.nbk_selftest_math.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp]
    lib.nbk_knn_prefix.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.nbk_fk_batch_host.argtypes = [vp, vp, i64, vp, i32, vp, vp]
    lib.nbk_validity_batch_host.argtypes = [vp, vp, i64, f64, vp]
    lib.nbk_model_num_pairs.argtypes = [vp]
    lib.nbk_validity_scalar_host.argtypes = [vp, vp, f64, vp]
    lib.nbk_edge_validity_scalar_host.argtypes = [vp, vp, vp, f64, f64, f64, i32, f64, vp, vp, vp]
    lib.nbk_cloud_create.argtypes = [i64, vp, f64, vp, C.POINTER(C.c_void_p)]
    lib.nbk_cloud_destroy.argtypes = [vp]
    lib.nbk_cloud_destroy.restype = None
    lib.nbk_cloud_set_points.argtypes = [vp, vp, i64, f64, vp]
    lib.nbk_cloud_status.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.nbk_cloud_validity_batch.argtypes = [vp, vp, vp, i64, f64, vp, i32, vp, vp, vp]
    lib.nbk_cloud_clearance_batch.argtypes = [vp, vp, vp, i64, f64, vp, vp, vp, vp, vp]
    lib.nbk_cloud_cells_host.argtypes = [vp, f64, vp, vp, i64, vp]
    lib.nbk_records_cloud_batch.argtypes = [vp, vp, vp, i64, f64, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.nbk_edge_cloud_workspace_bytes.argtypes = [i64]
    lib.nbk_edge_cloud_workspace_bytes.restype = i64
    lib.nbk_edge_cloud_validity_batch.argtypes = [vp, vp, vp, vp, vp, i64, f64, f64, i32, f64, vp, i32, vp, vp, vp, vp, i64, vp]
    lib.nbk_edge_cloud_continuous_batch.argtypes = [vp, vp, vp, vp, vp, i64, f64, i32, f64, i32, f64, f64, vp, i32, vp, vp, vp, vp, vp]
    lib.nbk_edge_shape_motion_bounds_host.argtypes = [C.POINTER(ModelDesc), vp, vp, i64, vp]
    lib.nbk_spline_cloud_workspace_bytes.argtypes = [i64]
    lib.nbk_spline_cloud_workspace_bytes.restype = i64
    lib.nbk_spline_cloud_validity_batch.argtypes = [vp, vp, vp, i64, i32, i32, vp, f64, f64, vp, i32, vp, vp, vp, vp, i64, vp]
    lib.nbk_spline_cloud_continuous_batch.argtypes = [vp, vp, vp, i64, i32, i32, vp, f64, i32, f64, f64, vp, i32, vp, vp, vp, vp]
    lib.nbk_spline_shape_motion_bounds_host.argtypes = [C.POINTER(ModelDesc), vp, i64, i32, i32, vp, vp]
    lib.nbk_frame_cloud_backproject.argtypes = [vp, i32, i32, i32, f64, f64, f64, f64, f64, vp, f64, f64, vp, vp, vp]
    lib.nbk_frame_cloud_backproject_host.argtypes = [vp, i32, i32, i32, f64, f64, f64, f64, f64, vp, f64, f64, vp, vp]
    lib.nbk_frame_cloud_self_filter.argtypes = [vp, vp, vp, i64, f64, f64, vp, vp, vp]
    lib.nbk_frame_cloud_self_filter_lds_bytes.argtypes = [i32]
    lib.nbk_frame_cloud_self_filter_lds_bytes.restype = i64
    lib.nbk_frame_cloud_set_points.argtypes = [vp, vp, vp, i64, f64, vp]
    lib.nbk_frame_cloud_count.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.nbk_frame_cloud_carve.argtypes = [vp, i32, i32, i32, f64, f64, f64, f64, f64, vp, f64, f64, f64, i32, vp, i64, vp, vp]
    lib.nbk_frame_cloud_carve_host.argtypes = [vp, i32, i32, i32, f64, f64, f64, f64, f64, vp, f64, f64, f64, i32, vp, i64, vp]
    lib.nbk_frame_cloud_novel.argtypes = [vp, vp, i64, f64, vp, vp, vp]
    lib.nbk_frame_cloud_append_workspace_bytes.argtypes = [i64, i64]
    lib.nbk_frame_cloud_append_workspace_bytes.restype = i64
    lib.nbk_frame_cloud_append.argtypes = [vp, vp, i64, vp, vp, i64, vp, vp, vp, i64, vp]
    lib.nbk_render_depth_lds_bytes.argtypes = [i32]
    lib.nbk_render_depth_lds_bytes.restype = i64
    lib.nbk_render_ray_spans_host.argtypes = [i32, i32, f64, f64, f64, f64, vp, vp, vp, i32, f64, f64, vp, vp]
    lib.nbk_render_depth_batch.argtypes = [vp, vp, i64, vp, i64, i64, i32, i32, f64, f64, f64, f64, f64, f64, f64, i32, vp, i32, C.c_float,
                                           vp, vp, vp, vp]
    lib.nbk_held_locals_host.argtypes = [vp, vp, vp, i32, vp]
    lib.nbk_held_create.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, i32, vp, vp, C.POINTER(C.c_void_p)]
    lib.nbk_held_destroy.argtypes = [vp]
    lib.nbk_held_destroy.restype = None
    lib.nbk_held_validity_batch.argtypes = [vp, vp, vp, i64, vp, i64, f64, i32, vp, vp, vp]
    lib.nbk_edge_held_workspace_bytes.argtypes = [i64]
    lib.nbk_edge_held_workspace_bytes.restype = i64
    lib.nbk_edge_held_validity_batch.argtypes = [vp, vp, vp, vp, vp, i64, f64, f64, i32, f64, vp, i32, vp, vp, vp, vp, i64, vp]
    lib.nbk_held_item_count.argtypes = [vp]
    lib.nbk_held_items.argtypes = [vp, vp]
    lib.nbk_held_distances_batch.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp]
    lib.nbk_held_records_batch.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp, vp, vp]
    lib.nbk_held_records_items.argtypes = [vp, vp, vp, i64, vp, i64, vp, i64, vp, vp, vp, vp]
    lib.nbk_edge_held_continuous_batch.argtypes = [vp, vp, vp, vp, vp, i64, f64, i32, f64, i32, f64, vp, i32, vp, vp, vp, vp, vp]
    lib.nbk_spline_held_continuous_batch.argtypes = [vp, vp, vp, i64, i32, i32, vp, f64, i32, f64, vp, i32, vp, vp, vp, vp]
    lib.nbk_spline_held_workspace_bytes.argtypes = [i64]
    lib.nbk_spline_held_workspace_bytes.restype = i64
    lib.nbk_spline_held_validity_batch.argtypes = [vp, vp, vp, i64, i32, i32, vp, f64, f64, vp, i32, vp, vp, vp, vp, i64, vp]
    held_args = [C.POINTER(ModelDesc), i32, vp, vp, i32, vp, vp, vp, i32, vp, vp]       # the descriptor, then nbk_held_create's
    lib.nbk_edge_held_motion_bounds_host.argtypes = held_args + [vp, vp, i64, vp]
    lib.nbk_spline_held_motion_bounds_host.argtypes = held_args + [vp, i64, i32, i32, vp, vp]
    hull_args = [i32, vp, vp, vp, vp]                 # n_hulls, hull_vert_begin, hull_verts, hull_face_begin, hull_planes
    lib.nbk_held_create_hulls.argtypes = [vp] + held_args[1:] + hull_args + [C.POINTER(C.c_void_p)]
    lib.nbk_edge_held_motion_bounds_hulls_host.argtypes = held_args + hull_args + [vp, vp, i64, vp]
    lib.nbk_spline_held_motion_bounds_hulls_host.argtypes = held_args + hull_args + [vp, i64, i32, i32, vp, vp]
    lib.nbk_held_cloud_validity_batch.argtypes = [vp, vp, vp, vp, i64, vp, i64, f64, i32, vp, vp, vp]
    lib.nbk_held_cloud_clearance_batch.argtypes = [vp, vp, vp, vp, i64, vp, i64, f64, vp, vp, vp, vp]
    lib.nbk_held_cloud_records_batch.argtypes = [vp, vp, vp, vp, i64, vp, i64, f64, i32, vp, vp, vp, vp, vp, vp]
    lib.nbk_edge_held_cloud_workspace_bytes.argtypes = [i64]
    lib.nbk_edge_held_cloud_workspace_bytes.restype = i64
    lib.nbk_edge_held_cloud_validity_batch.argtypes = [vp, vp, vp, vp, vp, vp, i64, f64, f64, i32, f64, vp, i32, vp, vp, vp, vp, i64, vp]
    lib.nbk_spline_held_cloud_workspace_bytes.argtypes = [i64]
    lib.nbk_spline_held_cloud_workspace_bytes.restype = i64
    lib.nbk_spline_held_cloud_validity_batch.argtypes = [vp, vp, vp, vp, i64, i32, i32, vp, f64, f64, vp, i32, vp, vp, vp, vp, i64, vp]
    lib.nbk_edge_held_cloud_continuous_batch.argtypes = [vp, vp, vp, vp, vp, vp, i64, f64, i32, f64, i32, f64, f64, vp, i32, vp, vp, vp, vp,
                                                         vp]
    lib.nbk_spline_held_cloud_continuous_batch.argtypes = [vp, vp, vp, vp, i64, i32, i32, vp, f64, i32, f64, f64, vp, i32, vp, vp, vp, vp]
    held_shape_args = held_args[:8]                                                     # (no world list, no robot set)
    lib.nbk_edge_held_shape_motion_bounds_host.argtypes = held_shape_args + [vp, vp, i64, vp]
    lib.nbk_spline_held_shape_motion_bounds_host.argtypes = held_shape_args + [vp, i64, i32, i32, vp, vp]
    lib.nbk_held_set_cloud_hulls.argtypes = [vp, i32]
    lib.nbk_edge_held_shape_motion_bounds_hulls_host.argtypes = held_shape_args + hull_args + [vp, vp, i64, vp]
    lib.nbk_spline_held_shape_motion_bounds_hulls_host.argtypes = held_shape_args + hull_args + [vp, i64, i32, i32, vp, vp]
    lib.nbk_debug_set_option.argtypes = [C.c_char_p, i64]
    lib.nbk_debug_narrow_variant.argtypes = [vp, f64]
    lib.nbk_debug_last_tiling.argtypes = [vp, C.POINTER(i64)]
    _lib = lib
    return lib


# tuning / diagnostic switches of the library (process-wide; seeded once from the NBK_* environment variables when the library
# is loaded, never read again): name -> default.  None of them changes a result.
DEBUG_OPTIONS = {"two_kernel_min_b": 1, "edge_batch_min_e": 1, "no_reg_broad": 0, "f64_broad": 0, "jac_two_sweep": 0,
                 "closest_brute": 0, "narrow_parts_max": 16, "queue_budget": 1 << 30, "pipeline_tiles": 1, "pipe_tile": 1 << 20, "fk_lds_q": 0}


def set_debug_option(name: str, value: int):
    check(load().nbk_debug_set_option(name.encode(), int(value)), f"nbk_debug_set_option({name})")


class debug_option:
    """``with debug_option("two_kernel_min_b", 10**9): ...`` -- route calls through another kernel path (tests, tools)."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        set_debug_option(self.name, self.value)

    def __exit__(self, *exc):
        set_debug_option(self.name, DEBUG_OPTIONS[self.name])
        return False


def check(status: int, what: str):
    if status != NBK_OK:
        lib = load()
        msg = lib.nbk_status_string(status).decode()
        detail = lib.nbk_last_error().decode() if status == -3 else ""
        raise NbkError(f"{what} failed: {STATUS.get(status, status)} ({msg}) {detail}".strip())
