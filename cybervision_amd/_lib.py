"""ctypes binding of libcvhip.so — one Python function per C-ABI entry point (include/cvhip.h).

Fails loudly when the extension has not been built: there is no fallback path.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libcvhip.so"
_lib = None


class CvhipError(RuntimeError):
    """Non-zero return of a cvhip_* call; mirrors GpuError::Internal (gpu/vulkan.rs:1204-1272)."""

    def __init__(self, code: int, where: str, msg: str):
        super().__init__(f"{where}: {msg} (code {code})")
        self.code = code


PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_float)
MATCHES_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int)
_vp = C.c_void_p
_u32 = C.c_uint32

# name -> (restype, argtypes); kept in sync with include/cvhip.h (tests/test_abi.py checks it)
SIGNATURES = {
    "cvhip_last_error": (C.c_char_p, []),
    "cvhip_abi_version": (_u32, []),
    "cvhip_device_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(_vp)]),
    "cvhip_device_create_on_stream": (C.c_int, [C.c_int, C.c_int, _vp, C.POINTER(_vp)]),
    "cvhip_device_destroy": (None, [_vp]),
    "cvhip_device_name": (C.c_char_p, [_vp]),
    "cvhip_device_synchronize": (C.c_int, [_vp]),
    "cvhip_ctx_create": (C.c_int, [_vp, _u32, _u32, _u32, _u32, C.c_int, C.POINTER(C.c_double), C.POINTER(_vp)]),
    "cvhip_ctx_destroy": (None, [_vp]),
    "cvhip_correlate_images": (C.c_int, [_vp, _vp, _u32, _u32, _vp, _u32, _u32, C.c_float, C.c_int, C.c_int,
                                         PROGRESS_FN, _vp]),
    "cvhip_cross_check_filter": (C.c_int, [_vp, C.c_float, C.c_int]),
    "cvhip_correlate_level": (C.c_int, [_vp, _vp, _u32, _u32, _vp, _u32, _u32, C.c_float, C.c_int, PROGRESS_FN,
                                        _vp]),
    "cvhip_complete": (C.c_int, [_vp, _vp, _vp]),
    "cvhip_complete_dir": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "cvhip_complete_packed": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "cvhip_triangulate_affine": (C.c_int, [_vp, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cvhip_extend_tracks": (C.c_int, [_vp, _vp, C.c_uint64, _u32, _vp, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cvhip_triangulate_perspective": (C.c_int, [_vp, _vp, C.c_uint64, _u32, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp,
                                                C.POINTER(C.c_uint64), _vp, _vp, _vp, PROGRESS_FN, _vp]),
    "cvhip_ctx_set_row_shard": (C.c_int, [_vp, _u32, _u32, ALLGATHER_FN, _vp]),
    "cvhip_ctx_set_row_band": (C.c_int, [_vp, _u32, _u32]),
    "cvhip_rccl_unique_id": (C.c_int, [_vp]),
    "cvhip_rccl_create": (C.c_int, [_vp, _vp, _u32, _u32, C.POINTER(_vp)]),
    "cvhip_rccl_destroy": (None, [_vp]),
    "cvhip_rccl_allgather": (C.c_int, [_vp, _vp, C.c_uint64]),
    "cvhip_rccl_gather": (C.c_int, [_vp, _vp, C.c_uint64, _u32]),
    "cvhip_ctx_set_row_shard_rccl": (C.c_int, [_vp, _vp]),
    "cvhip_ctx_gather_bands_rccl": (C.c_int, [_vp, _vp, C.c_int]),
    "cvhip_ctx_level_grid": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u32), C.POINTER(_u32),
                                       C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "cvhip_ctx_set_profiling": (C.c_int, [_vp, C.c_int, C.c_int]),
    "cvhip_ctx_get_profile": (C.c_int, [_vp, C.POINTER(_u32), C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                        C.c_int]),
    "cvhip_ctx_get_kernel_times": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(_u32), C.c_int]),
    "cvhip_ctx_get_counters": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.c_int]),
    "cvhip_ctx_get_box_counters": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.c_int]),
    "cvhip_ctx_set_box_fold": (C.c_int, [_vp, C.c_int]),
    "cvhip_ctx_get_box_fold_counters": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.c_int]),
    "cvhip_ctx_set_row_lines": (C.c_int, [_vp, C.c_int]),
    "cvhip_ctx_get_row_lines_used": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "cvhip_ctx_set_range_mode": (C.c_int, [_vp, C.c_int]),
    "cvhip_ctx_set_exact_scores": (C.c_int, [_vp, C.c_int]),
    "cvhip_ctx_set_async_readback": (C.c_int, [_vp, C.c_int]),
    "cvhip_ctx_set_result_bands": (C.c_int, [_vp, C.c_uint32]),
    "cvhip_ctx_get_result_bands": (C.c_int, [_vp, C.POINTER(C.c_uint32)]),
    "cvhip_ctx_set_fused_finish": (C.c_int, [_vp, C.c_int]),
    "cvhip_ctx_set_search_version": (C.c_int, [_vp, C.c_int]),
    "cvhip_ctx_set_borrow_inputs": (C.c_int, [_vp, C.c_int]),
    "cvhip_ctx_set_fuse_level_calls": (C.c_int, [_vp, C.c_int]),
    "cvhip_ctx_set_stats_ahead": (C.c_int, [_vp, C.c_int]),
    "cvhip_downsample_box": (C.c_int, [_vp, _vp, _u32, _u32, _vp]),
    "cvhip_resize_lanczos3": (C.c_int, [_vp, _vp, _u32, _u32, _vp, _u32, _u32]),
    "cvhip_orb_extract": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, C.POINTER(_u32), PROGRESS_FN, _vp]),
    "cvhip_orb_extract_batch": (C.c_int, [_vp, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _vp, PROGRESS_FN, _vp]),
    "cvhip_orb_set_orientation_guard": (C.c_int, [_vp, C.c_double]),
    "cvhip_match_points": (C.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _u32, _u32, _vp, _vp, C.POINTER(_u32)]),
    "cvhip_ransac_affine": (C.c_int, [_vp, _vp, _u32, C.c_uint64, _vp, C.POINTER(_u32), _vp]),
    "cvhip_ransac_perspective": (C.c_int, [_vp, _vp, _u32, C.c_double, C.c_uint64, _u32, _vp, C.POINTER(_u32), _vp]),
    "cvhip_ransac_set_pencil": (C.c_int, [_vp, C.c_int]),
    "cvhip_ransac_set_lm_pipeline": (C.c_int, [_vp, C.c_int]),
    "cvhip_ransac_set_count_mfma": (C.c_int, [_vp, C.c_int]),
    "cvhip_ransac_set_in_order": (C.c_int, [_vp, C.c_int]),
    "cvhip_ransac_perspective_models": (C.c_int, [_vp, _vp, _u32, _vp, _u32, C.c_double, _vp]),
    "cvhip_ransac_affine_models": (C.c_int, [_vp, _vp, _u32, _vp, _u32, C.c_double, _vp]),
    "cvhip_fits_model": (C.c_int, [_vp, _vp, _vp, _u32, C.c_double, _vp]),
    "cvhip_ransac_round_score": (C.c_int, [_vp, _vp, _u32, _vp, _u32, C.c_double, _vp, _vp]),
    "cvhip_ransac_rounds_pick": (C.c_int, [_vp, _vp, _u32, _u32, _vp, _u32, C.c_double, _u32, _vp, C.POINTER(_u32),
                                           C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "cvhip_find_ransac": (C.c_int, [_vp, C.c_int, _vp, _u32, C.c_double, C.c_uint64, _vp, C.POINTER(_u32), _vp, PROGRESS_FN,
                                    MATCHES_FN, _vp]),
    "cvhip_optimize_perspective_f": (C.c_int, [_vp, _vp, _u32, _vp, _vp]),
    "cvhip_optimize_perspective_f_device": (C.c_int, [_vp, _vp, _vp, _u32, _vp, _vp]),
    "cvhip_ransac_score": (C.c_int, [_vp, _vp, _u32, _vp, _u32, C.c_double, _vp, _vp]),
    "cvhip_triangulate_perspective_cameras": (C.c_int, [_vp, _vp, C.c_uint64, _u32, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp,
                                                        _vp, _vp, _vp, C.POINTER(C.c_uint64), C.POINTER(_u32), _vp, _vp,
                                                        PROGRESS_FN, _vp]),
    "cvhip_extend_tracks_matches": (C.c_int, [_vp, _vp, C.c_uint64, _u32, _u32, _vp, C.c_uint64, _u32, _vp, _vp, _vp,
                                              C.c_uint64, C.POINTER(C.c_uint64)]),
    "cvhip_triangulate_tracks": (C.c_int, [_vp, _vp, C.c_uint64, _u32, _vp, _vp, _vp, _vp]),
    "cvhip_find_projection_matrix": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint64, _vp, C.POINTER(C.c_double), _vp,
                                               _vp]),
    "cvhip_recover_pose": (C.c_int, [_vp, _vp, C.c_uint64, _u32, _vp, _vp, _vp, _vp, _u32, _vp, _u32, C.c_uint64, _vp, _vp,
                                     _vp, C.POINTER(_u32), C.POINTER(C.c_double), C.POINTER(_u32), _vp, PROGRESS_FN,
                                     _vp]),
    "cvhip_recover_pose_models": (C.c_int, [_vp, _vp, C.c_uint64, _u32, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _vp, _u32, _vp,
                                            _vp, _vp, _vp]),
    "cvhip_merge_tracks": (C.c_int, [_vp, _vp, C.c_uint64, _u32, _u32, _u32, _u32, _vp, _vp, C.POINTER(C.c_uint64), _vp]),
    # max_points: (n, max_points, seed, points, tracks, m_cams, out_rows, out_points, out_tracks, out_n); (keys, n, m, out_rows, out_n)
    "cvhip_surface_subset": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _vp, _u32, _vp, _vp, _vp, C.POINTER(C.c_uint64)]),
    "cvhip_select_smallest_u64": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, _vp, C.POINTER(C.c_uint64)]),
    # the dense track table in device memory: (dev, m, reserve_rows, out); (t, out_rows, out_capacity, out_m, out_device_rows);
    # (t, rows, n); (t, first, n, out); (t, ctx, image1, image2, max_dimension2, out_counts[3]);
    # (t, image_index, width, height, out_stats[4]); (src, columns, k, out); (t, rows, k, out)
    "cvhip_tracks_create": (C.c_int, [_vp, _u32, C.c_uint64, C.POINTER(_vp)]),
    "cvhip_tracks_destroy": (None, [_vp]),
    "cvhip_tracks_info": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(_u32), C.POINTER(_vp)]),
    "cvhip_tracks_assign": (C.c_int, [_vp, _vp, C.c_uint64]),
    "cvhip_tracks_read": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _vp]),
    "cvhip_tracks_extend": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _vp]),
    "cvhip_tracks_merge": (C.c_int, [_vp, _u32, _u32, _u32, _vp]),
    "cvhip_tracks_select_columns": (C.c_int, [_vp, _vp, _u32, C.POINTER(_vp)]),
    "cvhip_tracks_gather": (C.c_int, [_vp, _vp, C.c_uint64, _vp]),
    # the mesh stage; the surface is (points, tracks, n, m, projection, r, t, image_dims) in every entry
    "cvhip_mesh_set_wide_threshold": (C.c_int, [_vp, _u32]),
    "cvhip_mesh_camera_points": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _u32, _vp, _vp, _vp, _vp, _u32, _vp, _vp, C.c_uint64,
                                           C.POINTER(C.c_uint64)]),
    "cvhip_mesh_depth_buffer": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _u32, _vp, _vp, _vp, _vp, _u32, _vp, C.c_uint64,
                                          C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cvhip_mesh_cull": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _u32, _vp, _vp, _vp, _vp, _u32, _vp, C.c_uint64, _vp, _vp]),
    "cvhip_mesh_merge": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, _vp, C.POINTER(C.c_uint64)]),
    "cvhip_mesh_depth_image": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _u32, _vp, _vp, _vp, _vp, _u32, C.c_double, _vp,
                                         C.c_uint64, _vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _vp, _vp,
                                         C.POINTER(C.c_uint64)]),
    # the mesh output: (points, tracks, n, m, images, image_offsets, image_dims, vertex_mode, out_scale, polygons, n_poly, ...)
    "cvhip_mesh_ply": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _u32, _vp, _vp, _vp, _u32, _vp, _vp, C.c_uint64, _vp, C.c_uint64,
                                 C.POINTER(C.c_uint64), _vp]),
    "cvhip_mesh_colour_map": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, C.c_double, C.c_double, _vp, _vp]),
    # the OBJ file image: cvhip_mesh_ply's arguments with polygon_cameras behind polygons and stem behind n_poly
    "cvhip_mesh_obj": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _vp, C.c_uint64, C.c_char_p, _vp,
                                 C.c_uint64, C.POINTER(C.c_uint64), _vp]),
    "cvhip_mesh_obj_mtl": (C.c_int, [C.c_char_p, _u32, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cvhip_f64_display": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, C.POINTER(C.c_uint64), _vp]),
    # the PNG file image: (pixels, width, height, channels, filter, out, cap, out_size, out_sections[3])
    "cvhip_png_encode": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, C.c_uint64, C.POINTER(C.c_uint64), _vp]),
    # the JPEG file image: (pixels, width, height, channels, quality, sampling, optimize, out, cap, out_size, out_sections[3]);
    # (out_stats[4])
    "cvhip_jpeg_encode": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, C.c_uint64, C.POINTER(C.c_uint64), _vp]),
    "cvhip_jpeg_encode_last_stats": (C.c_int, [_vp]),
    # the TIFF file image: (pixels, width, height, channels, compression, predictor, rows_per_strip, out, cap, out_size,
    # out_sections[3]); (out_stats[4]); (out_ticks[3])
    "cvhip_tiff_encode": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, C.c_uint64, C.POINTER(C.c_uint64), _vp]),
    "cvhip_tiff_encode_last_stats": (C.c_int, [_vp]),
    "cvhip_tiff_encode_last_phases": (C.c_int, [_vp]),
    # JPEG files in: (file, size, out_info[6]); (file, size, format, drop_rows, out, cap, out_size); (out_stats[4])
    "cvhip_jpeg_info": (C.c_int, [_vp, C.c_uint64, _vp]),
    "cvhip_jpeg_decode": (C.c_int, [_vp, _vp, C.c_uint64, _u32, _u32, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cvhip_jpeg_last_stats": (C.c_int, [_vp]),
    # progressive JPEG files in: (file, size, out_info[7]); cvhip_jpeg_decode's arguments; (out_stats[8])
    "cvhip_jpeg_progressive_info": (C.c_int, [_vp, C.c_uint64, _vp]),
    "cvhip_jpeg_progressive_decode": (C.c_int, [_vp, _vp, C.c_uint64, _u32, _u32, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cvhip_jpeg_progressive_last_stats": (C.c_int, [_vp]),
    # TIFF files in: (file, size, out_info[12], out_scale[3]); (file, size, format, drop_rows, out, cap, out_size); (out_stats[4])
    "cvhip_tiff_info": (C.c_int, [_vp, C.c_uint64, _vp, _vp]),
    "cvhip_tiff_decode": (C.c_int, [_vp, _vp, C.c_uint64, _u32, _u32, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cvhip_tiff_last_stats": (C.c_int, [_vp]),
    # Deflate and tiled TIFF files in: (file, size, out_info[16], out_scale[3]); cvhip_tiff_decode's arguments; (out_stats[12])
    "cvhip_tiff_ext_info": (C.c_int, [_vp, C.c_uint64, _vp, _vp]),
    "cvhip_tiff_ext_decode": (C.c_int, [_vp, _vp, C.c_uint64, _u32, _u32, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cvhip_tiff_ext_last_stats": (C.c_int, [_vp]),
    # PNG files in: (file, size, out_info[8]); (file, size, format, drop_rows, out, cap, out_size); (out_stats[8])
    "cvhip_png_info": (C.c_int, [_vp, C.c_uint64, _vp]),
    "cvhip_png_decode": (C.c_int, [_vp, _vp, C.c_uint64, _u32, _u32, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cvhip_png_last_stats": (C.c_int, [_vp]),
    "cvhip_png_ext_info": (C.c_int, [_vp, C.c_uint64, _vp]),
    "cvhip_png_ext_decode": (C.c_int, [_vp, _vp, C.c_uint64, _u32, _u32, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cvhip_png_ext_last_stats": (C.c_int, [_vp]),
    # the Delaunay triangulation of a camera's points: (xy, k, out_faces, cap_faces, out_n_faces, out_stats)
    "cvhip_mesh_delaunay": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, C.POINTER(C.c_uint64), _vp]),
    "cvhip_mesh_delaunay_set_lane_cells": (C.c_int, [_vp, _u32]),
    "cvhip_mesh_delaunay_set_lattice": (C.c_int, [_vp, C.c_int]),
    "cvhip_mesh_delaunay_get_lattice": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "cvhip_mesh_delaunay_get_lattice_stars": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
}


def lib():
    """Load libcvhip.so (once).  Raises if it has not been built — no fallback."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(python -m cybervision_amd.build, or __graft_entry__.build()). There is no CPU fallback.")
        try:
            # torch bundles its own ROCm runtime; loading it FIRST makes libcvhip.so bind to that
            # same libamdhip64.so.7, so one process never holds two HIP runtimes (the second one
            # would see "no HIP GPUs").
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(str(LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the ABI symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc: int, where: str):
    if rc != 0:
        msg = lib().cvhip_last_error()
        raise CvhipError(rc, where, msg.decode("utf-8", "replace") if msg else "")


NULL_PROGRESS = PROGRESS_FN()
NULL_MATCHES = MATCHES_FN()
NULL_ALLGATHER = ALLGATHER_FN()
