"""ctypes mirror of include/vrt_api.h (structs and constants only; no library is loaded here)."""
import ctypes as C

import numpy as np

VRT_OK = 0
VRT_E_INVALID, VRT_E_DEVICE, VRT_E_STATE = -1, -2, -3

BUF_GBUF_DEPTH, BUF_GBUF_NORMAL, BUF_GBUF_POSITION, BUF_GBUF_MAT, BUF_GBUF_REFL_DEPTH = 1, 2, 3, 4, 5
BUF_HISTORY_DIFFUSE, BUF_HISTORY_SPECULAR, BUF_SKY_SCATTERING, BUF_SKY_TRANSMITTANCE, BUF_TRANS_LUT = 6, 7, 8, 9, 10
HIT_MISS, HIT_FLOOR, HIT_VOXEL = 0, 1, 2
RAY_ANY_HIT = 1
# vrt_ray / vrt_ray_hit (vrt_cast_rays): arrays of these go in and come out
RAY = np.dtype([("origin", np.float32, 3), ("t_max", np.float32), ("dir", np.float32, 3), ("flags", np.uint32)])
HIT = np.dtype([("t", np.float32), ("kind", np.int32), ("cell", np.int32, 3), ("normal", np.float32, 3), ("albedo", np.float32, 3),
                ("mat_id", np.int32)])
assert RAY.itemsize == 32 and HIT.itemsize == 48
# vrt_box_sweep / vrt_sweep_hit (vrt_sweep_boxes)
SWEEP_MISS, SWEEP_FLOOR, SWEEP_VOXEL, SWEEP_START = 0, 1, 2, 3
SWEEP_NO_FLOOR = 1
SWEEP_MAX_COORD = 64.0
BOX_SWEEP = np.dtype([("lo", np.float32, 3), ("flags", np.uint32), ("hi", np.float32, 3), ("reserved", np.uint32), ("move", np.float32, 3),
                      ("t_max", np.float32)])
SWEEP_HIT = np.dtype([("t", np.float32), ("kind", np.int32), ("cell", np.int32, 3), ("normal", np.float32, 3)])
assert BOX_SWEEP.itemsize == 48 and SWEEP_HIT.itemsize == 32
# vrt_triangle / vrt_voxelize_result (vrt_voxelize_triangles)
TRI_MAX_COORD = 8.0
TRIANGLE = np.dtype([("v0", np.float32, 3), ("voxel", np.uint32), ("v1", np.float32, 3), ("reserved0", np.uint32), ("v2", np.float32, 3),
                     ("reserved1", np.uint32)])
VOXELIZE_RESULT = np.dtype([("lo", np.int32, 3), ("hi", np.int32, 3), ("voxels", np.int64), ("invalid", np.int64)])
assert TRIANGLE.itemsize == 48 and VOXELIZE_RESULT.itemsize == 40
# vrt_distance_field
DIST_TO_EMPTY = 1
DIST_FAR = 0x7FFFFFFF
DIST_MAX_D2 = 195075
# vrt_label_result (vrt_label_components)
LABEL_EMPTY, LABEL_CONN_18, LABEL_CONN_26 = 1, 2, 4
LABEL_RESULT = np.dtype([("cells", np.int64), ("components", np.int32), ("reserved", np.int32)])
assert LABEL_RESULT.itemsize == 16
# vrt_voxel_move / vrt_move_result (vrt_move_voxels)
MOVE_ERASE_SOURCE, MOVE_KEEP_SOLID, MOVE_DRY_RUN, MOVE_IF_FREE = 1, 2, 4, 8
MOVE_M_MAX, MOVE_T_MAX = 1 << 20, 1 << 40
VOXEL_MOVE = np.dtype([("src_lo", np.int32, 3), ("src_hi", np.int32, 3), ("dst_lo", np.int32, 3), ("dst_hi", np.int32, 3), ("m", np.int32, 9),
                       ("select_value", np.int32), ("t", np.int64, 3), ("flags", np.uint32), ("reserved", np.uint32)])
MOVE_RESULT = np.dtype([("lo", np.int32, 3), ("hi", np.int32, 3), ("written", np.int64), ("blocked", np.int64), ("erased", np.int64)])
assert VOXEL_MOVE.itemsize == 120 and VOXEL_MOVE.fields["t"][1] == 88 and MOVE_RESULT.itemsize == 48
# vrt_path_ray / vrt_radiance (vrt_trace_radiance)
PATH_RAY = np.dtype([("origin", np.float32, 3), ("stream", np.uint32), ("dir", np.float32, 3), ("reserved", np.uint32)])
RADIANCE = np.dtype([("rgb", np.float32, 3), ("t", np.float32)])
RADIANCE_MAX_SAMPLES = 65536
assert PATH_RAY.itemsize == 32 and RADIANCE.itemsize == 16
# vrt_sensor / vrt_irradiance (vrt_gather_irradiance)
SENSOR = np.dtype([("pos", np.float32, 3), ("stream", np.uint32), ("normal", np.float32, 3), ("reserved", np.uint32)])
IRRADIANCE = np.dtype([("sky_rgb", np.float32, 3), ("sky", np.float32), ("sun_rgb", np.float32, 3), ("sun", np.float32)])
assert SENSOR.itemsize == 32 and IRRADIANCE.itemsize == 32
# vrt_probe / vrt_sh_probe (vrt_gather_probes)
PROBE = np.dtype([("pos", np.float32, 3), ("stream", np.uint32)])
SH_PROBE = np.dtype([("sh", np.float32, (9, 3)), ("sky", np.float32), ("sun_rgb", np.float32, 3), ("sun", np.float32)])
assert PROBE.itemsize == 16 and SH_PROBE.itemsize == 128


class VrtConfig(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("grid_res", C.c_int32),
        ("dx", C.c_float), ("voxel_edges", C.c_float), ("exposure", C.c_float),
        ("max_depth", C.c_int32), ("use_restir", C.c_int32), ("seed", C.c_uint32),
        ("sky_res", C.c_int32), ("device", C.c_int32),
        ("row_begin", C.c_int32), ("row_end", C.c_int32),
    ]


class VrtSceneParams(C.Structure):
    _fields_ = [
        ("floor_height", C.c_float), ("floor_color", C.c_float * 3), ("floor_material", C.c_int32),
        ("background_color", C.c_float * 3), ("light_direction", C.c_float * 3),
        ("light_cos_theta_max", C.c_float), ("light_color", C.c_float * 3), ("light_weight", C.c_float),
        ("use_physical_sky", C.c_int32), ("use_clouds", C.c_int32),
    ]


class VrtCamera(C.Structure):
    _fields_ = [
        ("view", C.c_float * 16), ("proj", C.c_float * 16), ("view_inv", C.c_float * 16), ("proj_inv", C.c_float * 16),
        ("pos", C.c_float * 3), ("jitter_index", C.c_uint32), ("camera_is_moving", C.c_int32),
        ("render_scale", C.c_float), ("max_accum_frames", C.c_float),
    ]


class VrtDenoiseParams(C.Structure):
    """vrt_denoise_params; the defaults are include/vrt_api.h's (a matter of taste, not validated on images)."""
    _fields_ = [("iterations", C.c_int32), ("plane_tolerance", C.c_float), ("sigma_l", C.c_float), ("full_at", C.c_float)]

    def __init__(self, iterations=5, plane_tolerance=0.25, sigma_l=0.5, full_at=64.0):
        super().__init__(int(iterations), float(plane_tolerance), float(sigma_l), float(full_at))


class VrtStats(C.Structure):
    _fields_ = [
        ("path_samples", C.c_uint64), ("rays", C.c_uint64), ("dda_iters", C.c_uint64),
        ("occupancy_queries", C.c_uint64), ("closest_hits", C.c_uint64), ("sky_lookups", C.c_uint64),
        ("render_ms", C.c_double), ("temporal_ms", C.c_double), ("gris_ms", C.c_double),
        ("render_launches", C.c_uint32), ("temporal_launches", C.c_uint32), ("gris_launches", C.c_uint32),
        ("pipeline_flags", C.c_uint32),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def declare(lib, prefix):
    """Attach argtypes/restype for the API shared by libvrt_hip.so (prefix 'vrt_') and the test
    oracle (prefix 'orc_').  Entry points one library lacks are skipped."""
    P = C.c_void_p

    def sig(name, res, *args):
        fn = getattr(lib, prefix + name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = list(args)

    sig("destroy", None, P)
    sig("upload_voxels", C.c_int, P, P, P)
    sig("upload_materials", C.c_int, P, P)
    sig("upload_cloud_texture", C.c_int, P, P)
    sig("set_scene", C.c_int, P, C.POINTER(VrtSceneParams))
    sig("set_camera", C.c_int, P, C.POINTER(VrtCamera))
    sig("prepare", C.c_int, P)
    sig("update_voxels", C.c_int, P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), P, P, C.c_int)
    sig("voxelize_triangles", C.c_int, P, C.c_int64, P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), P, C.c_int)
    sig("fill_triangles", C.c_int, P, C.c_int64, P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, P, C.c_int)
    sig("cast_rays", C.c_int, P, C.c_int64, P, P, C.c_int)
    sig("sweep_boxes", C.c_int, P, C.c_int64, P, P, C.c_int)
    sig("trace_radiance", C.c_int, P, C.c_int64, P, C.c_int, C.c_uint32, P, C.c_int)
    sig("gather_irradiance", C.c_int, P, C.c_int64, P, C.c_int, C.c_uint32, P, C.c_int)
    sig("gather_probes", C.c_int, P, C.c_int64, P, C.c_int, C.c_uint32, P, C.c_int)
    sig("fetch_voxels", C.c_int, P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), P, P, C.c_int)
    sig("distance_field", C.c_int, P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_uint32, P, P, C.c_int)
    sig("label_components", C.c_int, P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, P, P, C.c_int)
    sig("move_voxels", C.c_int, P, P, P, C.c_int, P)
    sig("sky_accumulate_clouds", C.c_int, P, C.c_int)
    sig("sky_compute_slice", C.c_int, P, C.c_int, C.c_int)
    sig("sky_accumulate_clouds_slice", C.c_int, P, C.c_int, C.c_int, C.c_int)
    sig("sky_table_io", C.c_int, P, C.c_int, C.c_int, C.c_int, P, C.c_int)
    sig("accumulate", C.c_int, P, C.c_int)
    sig("reset", C.c_int, P)
    sig("end_frame", C.c_int, P)
    sig("fetch_hdr", C.c_int, P, P)
    sig("fetch_hdr_device", C.c_int, P, P)
    sig("fetch_hdr_device_async", C.c_int, P, P)
    sig("set_stream", C.c_int, P, P)
    sig("reserve_cus", C.c_int, P, C.c_int)
    sig("fetch_ldr", C.c_int, P, P)
    sig("fetch_hdr_async", C.c_int, P, P, C.c_int)
    sig("fetch_ldr_async", C.c_int, P, P, C.c_int)
    sig("fetch_ldr8_async", C.c_int, P, P, C.c_int)
    sig("fetch_wait", C.c_int, P, C.c_int)
    sig("host_alloc", C.c_int, P, C.c_uint64, C.POINTER(C.c_void_p))
    sig("host_free", C.c_int, P, P)
    sig("set_hdr_targets", C.c_int, P, C.POINTER(C.c_void_p), C.c_int)
    sig("hdr_targets_written", C.c_int, P, C.POINTER(C.c_uint64))
    sig("fetch_buffer", C.c_int, P, C.c_int, P)
    sig("denoise", C.c_int, P, C.POINTER(VrtDenoiseParams), P, C.c_int)
    sig("sync", C.c_int, P)
    sig("get_stats", C.c_int, P, C.POINTER(VrtStats))
    sig("last_error", C.c_char_p)
    sig("is_instrumented", C.c_int)
    sig("set_reference_indexing", C.c_int, P, C.c_int)
    sig("set_row_stripes", C.c_int, P, C.c_int, C.c_int, C.c_int)
    sig("set_history_exchange", C.c_int, P, C.c_int)
    sig("history_rows_io", C.c_int, P, C.c_int, C.c_int, P, C.c_int)
