"""ctypes binding of libpcr.so (the C ABI declared in include/pcr_api.h).

The library is built in-tree (``pointcloudregistration_amd/libpcr.so``) by
``__graft_entry__.build()`` / ``make -C pointcloudregistration_amd/csrc``.
There is deliberately no fallback: if the HIP library is missing or fails to
load, every op raises ``PcrError`` (the product never routes through a CPU
path or the test oracle).
"""
from __future__ import annotations

import atexit
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PCR_LIB", os.path.join(_HERE, "libpcr.so"))

PCR_OK = 0


class PcrError(RuntimeError):
    """Raised when libpcr is unavailable or a libpcr call fails."""


_lib = None
_lock = threading.Lock()

_p = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_f32 = ctypes.c_float
_f64 = ctypes.c_double
_u64 = ctypes.c_uint64



class RansacParams(ctypes.Structure):
    """pcr_ransac_params (include/pcr_api.h)."""
    _fields_ = [("max_correspondence_distance", _f64), ("edge_length_ratio", _f64),
                ("distance_check", _f64), ("confidence", _f64), ("max_iteration", _i32),
                ("ransac_n", _i32), ("mutual_filter", _i32), ("reserved", _i32), ("seed", _u64)]


class IcpParams(ctypes.Structure):
    """pcr_icp_params (include/pcr_api.h)."""
    _fields_ = [("max_correspondence_distance", _f64), ("relative_fitness", _f64),
                ("relative_rmse", _f64), ("max_iteration", _i32), ("reserved", _i32)]


class IcpPlaneParams(ctypes.Structure):
    """pcr_icp_plane_params (include/pcr_api.h)."""
    _fields_ = [("kernel", _i32), ("reserved", _i32), ("k", _f64)]


class PointNetLayers(ctypes.Structure):
    """pcr_pointnet_layers (include/pcr_api.h): one branch's folded weights, device pointers."""
    _fields_ = [(n, _p) for n in ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")]


class PointNetWeights(ctypes.Structure):
    """pcr_pointnet_weights (include/pcr_api.h)."""
    _fields_ = [("stn", PointNetLayers), ("main", PointNetLayers)]


class GroupMlpNet(ctypes.Structure):
    """pcr_group_mlp_net (include/pcr_api.h): a host struct of device pointers."""
    _fields_ = [("layers", _i32), ("width", _i32 * 3), ("w", _p * 3), ("gamma", _p * 3), ("beta", _p * 3),
                ("y", _p * 3), ("stats", _p * 3)]


class UnaryArgs(ctypes.Structure):
    """pcr_unary_args (include/pcr_api.h): a host struct of device pointers."""
    _fields_ = [("n", _i32), ("m0", _i32), ("c0", _i32), ("c1", _i32), ("cout", _i32), ("x0", _p), ("ld0", _i64),
                ("g0", _p), ("x1", _p), ("ld1", _i64), ("w", _p), ("bias", _p), ("norm", _i32), ("eps", _f64),
                ("act", _i32), ("slope", _f32), ("res", _p), ("out", _p), ("y", _p), ("stats", _p)]


class PointwiseArgs(ctypes.Structure):
    """pcr_pointwise_args (include/pcr_api.h): a host struct of device pointers."""
    _fields_ = [("b", _i32), ("n", _i32), ("nsrc", _i32), ("cout", _i32), ("c", _i32 * 5), ("src", _p * 5),
                ("src_bs", _i64 * 5), ("src_cs", _i64 * 5), ("sub", _p * 5), ("sub_bs", _i64 * 5),
                ("sub_cs", _i64 * 5), ("w", _p), ("w_ld", _i64), ("bias", _p), ("cbias", _p), ("gw", _i32), ("eps", _f64),
                ("gamma", _p), ("beta", _p), ("act", _i32), ("slope", _f32), ("res", _p), ("res_bs", _i64),
                ("res_cs", _i64), ("out", _p), ("out_bs", _i64), ("out_cs", _i64), ("cmax", _p), ("y", _p),
                ("stats", _p)]


_rp = ctypes.POINTER(RansacParams)
_ip = ctypes.POINTER(IcpParams)
_ipp = ctypes.POINTER(IcpPlaneParams)

# name -> argtypes (restype is always c_int); keep in sync with include/pcr_api.h
SIGNATURES = {
    "pcr_nnd_forward": [_p, _p, _i32, _i32, _i32, _p, _p, _p, _p, _p],
    "pcr_nnd_backward": [_p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _p, _p, _p],
    "pcr_set_workspace_context": [_i32],
    "pcr_set_concurrency": [_i32],
    "pcr_nnd_forward_ragged": [_p, _p, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p],
    "pcr_nnd_forward_f64": [_p, _p, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p],
    "pcr_feature_match": [_p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p],
    "pcr_feature_correspondences": [_p, _p, _i32, _i32, _i32, _i32, _p, _p, _i32, _i32, _p, _p, _p, _p],
    "pcr_correspondences": [_p, _p, _i32, _i32, _i32, _p, _p, _i32, _i32, _p, _p, _p],
    "pcr_ransac_batch": [_p, _p, _i32, _i32, _i32, _p, _p, _p, _p, _i32, _p, _rp, _p, _p, _p,
                         _p, _p, _p],
    "pcr_register_feature_ransac": [_p, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _rp,
                                    _p, _p, _p, _p, _p, _p],
    "pcr_icp_batch": [_p, _p, _i32, _i32, _i32, _p, _p, _p, _ip, _p, _p, _p, _p, _p],
    "pcr_icp_plane_batch": [_p, _p, _p, _i32, _i32, _i32, _p, _p, _p, _ip, _ipp, _p, _p, _p, _p, _p],
    "pcr_radius_nn": [_p, _i32, _i32, _p, _p, _i32, _p, _f64, _p, _p, _p],
    "pcr_procrustes_batch": [_p, _p, _p, _i32, _i32, _i32, _f64, _p, _p],
    "pcr_procrustes_batch_f64": [_p, _p, _p, _i32, _i32, _i32, _f64, _p, _p],
    "pcr_lrf_count": [_p, _i32, _i32, _p, _p, _i32, _p, _f64, _p, _p],
    "pcr_lrf_compute": [_p, _i32, _i32, _p, _p, _i32, _p, _f64, _i32, _p, _i32, _p, _p, _p, _p],
    "pcr_ndp_warp": [_p, _i32, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _p],
    "pcr_grid_subsample": [_p, _i32, _p, _i32, _p, _i32, _f32, _i32, _p, _p, _p, _p, _p],
    "pcr_voxel_map_order": [_p, _i32, _p],
    "pcr_voxel_down_sample": [_p, _i32, _p, _i32, _f64, _p, _p, _p, _p, _p, _p, _p, _p],
    "pcr_voxel3i_map_order": [_p, _i32, _p],
    "pcr_legacy_choice_batch": [_p, _p, _p, _i32, _i32, _p],
    "pcr_vote_apply": [_p, _i32, _p, _p, _p, _i32, _f64, _p, _p, _p, _p, _i32, _p, _p],
    "pcr_radius_count": [_p, _i32, _p, _i32, _p, _p, _i32, _f32, _p, _p, _p],
    "pcr_radius_neighbors": [_p, _i32, _p, _i32, _p, _p, _i32, _f32, _i32, _p, _p, _p],
    "pcr_transform_batch": [_p, _i32, _i32, _p, _p, _p],
    "pcr_ndp_control": [_p, _p, _f64, _i32, _f64, _p],
    "pcr_adam_masked": [_p, _i32, _i32, _p, _f64, _f64, _f64, _f64, _p],
    "pcr_set_gate": [_p],
    "pcr_featmut_debug_copy": [_p, _i64, _p],
    "pcr_coop_probe": [_p, _i32, _i32, _p],
    "pcr_ndp_train_forward": [_p, _p],
    "pcr_ndp_train_backward": [_p, _p, _i32, _p, _p],
    "pcr_ndp_chamfer_glue": [_p, _i32, _p, _i32, _p, _i32, _f64, _f64, _p, _p, _p, _p, _p, _i32, _p],
    "pcr_ndp_chamfer_prepare": [_p, _p, _p],
    "pcr_ndp_chamfer_step": [_p, _p],
    "pcr_ndp_chamfer_loss": [_p, _i32, _p, _i32, _p, _i32, _f64, _f64, _p, _p, _p, _i32, _p, _f64, _i32,
                             _f64, _p, _p],
    "pcr_ndp_ldmk_loss": [_p, _p, _i32, _p, _i32, _p, _i32, _p, _i32, _f64, _f64, _f64, _p, _p, _p, _i32, _p,
                          _f64, _i32, _f64, _p, _p],
    "pcr_pipeline_step": [_p, _p, _p, _p],
    "pcr_pipeline_records": [_p, _p],
    "pcr_hybrid_search": [_p, _i32, _i32, _p, _f64, _i32, _p, _p, _p, _p],
    "pcr_estimate_normals": [_p, _i32, _i32, _p, _f64, _i32, _p, _p, _p],
    "pcr_compute_fpfh": [_p, _p, _i32, _i32, _p, _f64, _i32, _p, _p, _p, _p],
    "pcr_fps": [_p, _p, _i32, _i32, _i32, _p, _p],
    "pcr_ball_query": [_p, _p, _i32, _i32, _i32, _f32, _i32, _p, _p, _p],
    "pcr_group_ppf": [_p, _p, _i32, _i32, _f32, _i32, _i32, _p, _p, _p],
    "pcr_knn_graph": [_p, _i32, _i32, _i32, _p, _p, _p],
    "pcr_edge_features": [_p, _p, _i32, _i32, _i32, _i32, _i32, _p, _p],
    "pcr_similarity_topk": [_p, _p, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p],
    "pcr_tfmr_select": [_p, _p, _p, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p],
    "pcr_cpd_estep": [_p, _p, _i32, _i32, _i32, _p, _p, _p, _p, _f64, _p, _p, _p, _p, _p, _p],
    "pcr_cpd_register": [_p, _p, _i32, _i32, _i32, _p, _p, _i32, _f64, _i32, _f64, _p, _p, _p, _p, _p, _p, _p,
                         _p, _p],
    "pcr_kpconv_forward": [_p, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _i32, _i32, _i32, _f32, _i32, _p, _p,
                           _p],
    "pcr_neighbor_max": [_p, _p, _i32, _i32, _i32, _i32, _i32, _p, _p],
    "pcr_attention_forward": [_p, _i64, _i64, _i64, _p, _i64, _i64, _i64, _p, _i64, _i64, _i64, _p, _i64, _i64,
                              _i64, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _p, _p],
    "pcr_offset_attention_forward": [_p, _i64, _i64, _p, _i64, _i64, _p, _i64, _i64, _p, _i64, _p, _i64, _i64,
                                     _i32, _i32, _i32, _i32, _p, _p],
    "pcr_pointnet_forward": [_p, _i64, _i64, _i64, _i32, _i32, ctypes.POINTER(PointNetWeights), _i32, _i32, _i32,
                             _p, _p, _p, _p, _p, _p, _p, _p],
    "pcr_edge_conv": [_p, _i64, _i64, _i64, _p, _i32, _i32, _i32, _i32, _i32, _p, _f64, _f32, _i32, _p, _p, _p, _p,
                      _p],
    "pcr_group_mlp": [_p, _i32, _i32, _i32, _i32, ctypes.POINTER(GroupMlpNet), _i32, _f64, _f32, _i32, _p, _p, _p],
    "pcr_unary_forward": [ctypes.POINTER(UnaryArgs), _p, _p],
    "pcr_pointwise_forward": [ctypes.POINTER(PointwiseArgs), _p, _p],
}

_pi64 = ctypes.POINTER(_i64)
# name -> (restype, argtypes) of every entry point that does not return a pcr status as c_int
# through SIGNATURES: sizes, counters, the profile, the error text, teardown
OTHER_SIGNATURES = {
    "pcr_last_error": (ctypes.c_char_p, []),
    "pcr_version": (ctypes.c_int, []),
    "pcr_workspace_release": (ctypes.c_int, []),
    "pcr_profile_enable": (None, [_i32]),
    "pcr_profile_read": (ctypes.c_int, [_i32, ctypes.POINTER(_f64), _pi64, _i32]),
    "pcr_featnn_rescan_rows": (ctypes.c_int, [_pi64, _pi64, _i32]),
    "pcr_featnn_fallback_rows": (ctypes.c_int, [_pi64, _pi64, _i32]),
    "pcr_featnn_image_chunks": (ctypes.c_int, [ctypes.POINTER(_i32)]),
    "pcr_ndp_train_partial_floats": (_i64, [_i32] * 4),
    "pcr_ndp_train_partial_floats_head": (_i64, [_i32] * 5),
    "pcr_ndp_head_rows": (_i32, [_i32] * 2),
    "pcr_ndp_chamfer_scratch_bytes": (_i64, [_i32] * 2),
    "pcr_ndp_loss_scratch_bytes": (_i64, []),
    "pcr_ndp_ldmk_loss_scratch_bytes": (_i64, []),
    "pcr_ndp_chamfer_gacc_words": (_i64, [_i32]),
    "pcr_ndp_chamfer_max_points": (_i32, []),
    "pcr_tfmr_scratch_bytes": (_i64, [_i32] * 5),
    "pcr_cpd_scratch_bytes": (_i64, [_i32] * 3),
    "pcr_attention_scratch_bytes": (_i64, [_i32] * 6),
    "pcr_offset_attention_scratch_bytes": (_i64, [_i32] * 4),
    "pcr_pointnet_scratch_bytes": (_i64, [_i32] * 3),
    "pcr_edge_conv_scratch_bytes": (_i64, [_i32] * 5),
    "pcr_group_mlp_scratch_bytes": (_i64, [_i32] * 7),
    "pcr_unary_scratch_bytes": (_i64, [_i32] * 2),
    "pcr_pointwise_scratch_bytes": (_i64, [_i32] * 3),
    "pcr_shutdown": (ctypes.c_int, []),
}


def load():
    """Load libpcr.so once; raise PcrError (no fallback) if it cannot be loaded."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise PcrError(
                f"libpcr.so not found at {LIB_PATH}; build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C pointcloudregistration_amd/csrc`")
        try:
            lib = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover - depends on the box
            raise PcrError(f"failed to load {LIB_PATH}: {e}") from e
        for name, args in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = ctypes.c_int
            fn.argtypes = args
        for name, (res, args) in OTHER_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        # free the library's device objects (workspace, profiling events) at
        # interpreter exit, before torch's and the HIP runtime's own teardown
        # (round 3 saw a crash in exit() after a profiled run)
        atexit.register(shutdown)
        return lib


def exported_symbols():
    return list(OTHER_SIGNATURES) + list(SIGNATURES)


PROF_FEAT_SCREEN, PROF_NND_FWD, PROF_RANSAC_VALIDATE, PROF_ICP, PROF_RANSAC_HYP = 0, 1, 2, 3, 4
PROF_FEAT_RESCAN, PROF_FEAT_PACK, PROF_NND_GRID, PROF_FEAT_SCREEN2 = 5, 6, 7, 8
PROF_FEAT_SCREEN1B, PROF_FEAT_SCREEN2B = 9, 10   # the 3-term screens behind the 1-term ones
PROF_FEAT_REGROUP = 11   # featnn_regroup9 + featnn_finish9 (both passes)
PROF_SLOTS = 12   # pcr_internal.h kProfSlots


# bumped by every shutdown(): a HIP graph captured before it points at freed
# workspace buffers and must not be replayed (pipeline.PairPipeline re-captures)
_generation = 0


def generation():
    return _generation


def shutdown():
    """pcr_shutdown(): synchronise and free the library's per-device workspace and
    profiling events (idempotent; the library stays usable and re-allocates on
    the next call).  Graphs captured before it must not be replayed: the
    generation counter tells their owners.  Registered with atexit when the
    library is loaded."""
    global _generation
    if _lib is not None:
        _generation += 1
        _lib.pcr_shutdown()


def profile_enable(on=True):
    load().pcr_profile_enable(1 if on else 0)


def profile_read(pid, reset=True):
    """(total_ms, launches) of kernel slot `pid` since the last reset."""
    ms, cnt = _f64(0.0), _i64(0)
    rc = load().pcr_profile_read(pid, ctypes.byref(ms), ctypes.byref(cnt), 1 if reset else 0)
    if rc != PCR_OK:
        raise PcrError(load().pcr_last_error().decode())
    return ms.value, cnt.value


def featnn_rescan_rows(reset=True):
    """(rows12, rows21) sent to the exact feature-NN rescan since the last reset."""
    a, b = _i64(0), _i64(0)
    rc = load().pcr_featnn_rescan_rows(ctypes.byref(a), ctypes.byref(b), 1 if reset else 0)
    if rc != PCR_OK:
        raise PcrError(load().pcr_last_error().decode())
    return a.value, b.value


def featnn_fallback_rows(reset=True):
    """(rows12, cols21) the 1-term feature screens left to the 3-term ones since
    the last reset."""
    a, b = _i64(0), _i64(0)
    rc = load().pcr_featnn_fallback_rows(ctypes.byref(a), ctypes.byref(b), 1 if reset else 0)
    if rc != PCR_OK:
        raise PcrError(load().pcr_last_error().decode())
    return a.value, b.value


def featnn_image_chunks():
    """Chunks per tile of the last f16 feature screen's packed images: S =
    ceil(D / 16) for the compact image of the default correspondence route, 2 S + 1
    for the full one (every other route; PCR_FEAT_IMAGE=full forces it)."""
    c = _i32(0)
    rc = load().pcr_featnn_image_chunks(ctypes.byref(c))
    if rc != PCR_OK:
        raise PcrError(load().pcr_last_error().decode())
    return c.value


def call(name, *args):
    """Call a libpcr entry point; raise PcrError with pcr_last_error() on failure."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != PCR_OK:
        msg = lib.pcr_last_error().decode("utf-8", "replace")
        raise PcrError(f"{name} failed ({rc}): {msg}")
    return rc


def stream_handle(device=None):
    """hipStream_t of torch's current stream on `device` (0 = legacy default)."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
