"""vrt_plan.h compiled for the host (tests/emul/plan_emul.cpp) behind ctypes: the library's launch decisions without a GPU.  Test
infrastructure shared by tests/test_pipeline_plan_host.py and tests/poses.py."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_plan_emul.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(HERE, "emul", "plan_emul.cpp")
        deps = [src, os.path.join(ROOT, "voxel_rt2_amd", "csrc", "vrt_plan.h")]
        if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
            subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-unused-function", "-o", _SO, src],
                           check=True, capture_output=True)
        _lib = C.CDLL(_SO)
        _lib.plan_shape.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _lib.plan_period.argtypes = [C.c_int, C.c_int, C.c_longlong]
        _lib.plan_period.restype = C.c_uint
        _lib.plan_deep_items.restype = C.c_longlong
        _lib.plan_target.argtypes = [C.c_uint, C.c_int, C.c_int, C.c_int, C.c_uint]
        _lib.plan_target.restype = C.c_uint
        _lib.plan_wait.argtypes = [C.c_uint, C.c_uint, C.c_int, C.c_int]
        _lib.plan_set.argtypes = _lib.plan_lane.argtypes = [C.c_uint, C.c_int]
        _lib.plan_variant.argtypes = [C.POINTER(C.c_int)]
        _lib.plan_tri.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong, C.POINTER(C.c_longlong)]
    return _lib


def shape(items, queues, heavy=False, can_defer=True, streams=None, grid_div=None, pass_stream=None, defer4=None, defer8=None):
    """((n_streams, grid_div), defer_k, pass_on_render)"""
    knobs = (C.c_int * 5)(*[-100 if v is None else v for v in (streams, grid_div, pass_stream, defer4, defer8)])
    out = (C.c_int * 4)()
    lib().plan_shape(items, int(heavy), queues, int(can_defer), knobs, out)
    return (out[0], out[1]), out[3], bool(out[2])


VARIANT_BITS = ("pooled", "restir", "instr", "cull", "black_sun", "dense12", "share_primary")


def variant(width=1920, height=1080, max_depth=8, knob_render=-1, knob_cull=-1, use_restir=False, instrumented=False, count_as_timed=False,
            ref_oob=False, cull_active=True, dense_grid=False, light_emits=False, fused=4):
    """The names of the RenderVariant fields that plan_render_variant sets, as a set.  The defaults are bench config 2: S1 (sparse: there
    are rays to cull; scene.py's black default light) at 1080p, 8 bounces, 4 fused samples, the shipped switches."""
    args = (C.c_int * 13)(width, height, max_depth, knob_render, knob_cull, int(use_restir), int(instrumented), int(count_as_timed),
                          int(ref_oob), int(cull_active), int(dense_grid), int(light_emits), fused)
    bits = lib().plan_variant(args)
    assert 0 <= bits < 1 << len(VARIANT_BITS)
    return {name for k, name in enumerate(VARIANT_BITS) if bits >> k & 1}
