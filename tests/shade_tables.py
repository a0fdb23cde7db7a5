"""ctypes binding of tests/emul/_shade_tables.so (tests/emul/shade_tables_emul.cpp): the host build of the device headers'
tabulated shading terms beside the expressions they stand for, and the pooled-schedule emulation run with packed material rows.
Test tooling only."""
import ctypes as C
import os
import subprocess

import numpy as np

from voxel_rt2_amd._session import NativeSession

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_shade_tables.so")
_lib = None


def build(force=False):
    srcs = [os.path.join(HERE, "emul", f) for f in ("shade_tables_emul.cpp", "emul.cpp")]
    deps = srcs + [os.path.join(ROOT, "voxel_rt2_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "voxel_rt2_amd", "csrc")) if f.endswith(".h")]
    deps += [os.path.join(ROOT, "include", f) for f in os.listdir(os.path.join(ROOT, "include"))]
    if force or not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        # tests/emu.py's flags: no contraction, no fast-math; -mfma so that dm_fma is the hardware's single rounding
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared",
                        "-Wno-unknown-pragmas", "-o", _SO, srcs[0]], check=True, capture_output=True)
    return _SO


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class PackedRows(NativeSession):
    """emu.Emulated's pooled schedule with the render stage reading packed material rows (prefix emt_).
    derive_while_staging: the SceneData carries no derived table (its field left unset)."""

    def __init__(self, cfg, derive_while_staging=False):
        super().__init__(lib(), "emt_", cfg)
        self._mode = 1 if derive_while_staging else 0

    def accumulate(self, n):
        self._lib.emt_set_table_mode(C.c_int(self._mode))
        return super().accumulate(n)


def packed_rows(rows, derive_while_staging=False):
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 14)
    got, want = np.zeros_like(rows), np.zeros_like(rows)
    lib().emt_packed_rows(C.c_int(len(rows)), _p(rows), C.c_int(1 if derive_while_staging else 0), _p(got), _p(want))
    return got, want


def normal_bases():
    normals, got, want = np.zeros((64, 3), np.float32), np.zeros((64, 6), np.float32), np.zeros((64, 6), np.float32)
    fast = np.zeros(64, np.int32)
    lib().emt_normal_bases(_p(normals), _p(got), _p(want), _p(fast))
    return normals, got, want, fast


def bytes_over_255():
    got, want = np.zeros(256, np.float32), np.zeros(256, np.float32)
    id_got, id_want = np.zeros(256, np.int32), np.zeros(256, np.int32)
    lib().emt_bytes_over_255(_p(got), _p(want), _p(id_got), _p(id_want))
    return got, want, id_got, id_want


def unpack_albedo(enc):
    enc = np.ascontiguousarray(enc, dtype=np.uint32)
    got, want = np.zeros((len(enc), 3), np.float32), np.zeros((len(enc), 3), np.float32)
    lib().emt_unpack_albedo(C.c_int(len(enc)), _p(enc), _p(got), _p(want))
    return got, want


def cone_pdfs(cos_max, cos_theta):
    cos_max = np.ascontiguousarray(cos_max, dtype=np.float32)
    cos_theta = np.ascontiguousarray(cos_theta, dtype=np.float32)
    shape = (len(cos_max), len(cos_theta))
    got, unset, want = np.zeros(shape, np.float32), np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    lib().emt_cone_pdfs(C.c_int(shape[0]), _p(cos_max), C.c_int(shape[1]), _p(cos_theta), _p(got), _p(unset), _p(want))
    return got, unset, want


def texcoords(uv, W, H):
    uv = np.ascontiguousarray(uv, dtype=np.int32).reshape(-1, 2)
    got, want = np.zeros(uv.shape, np.float32), np.zeros(uv.shape, np.float32)
    lib().emt_texcoords(C.c_int(len(uv)), _p(uv), C.c_int(W), C.c_int(H), _p(got), _p(want))
    return got, want


def trace_counting_ties(session, rays, n_samples, first_frame):
    """vrt_trace_radiance's records from the host build over a PackedRows session's scene, and per ray the number of shaded vertices
    whose step normal has two or three non-zero components (the guard of ortho_basis_axis_normal)."""
    from voxel_rt2_amd import _abi
    rays = np.ascontiguousarray(rays, _abi.PATH_RAY)
    out, ties = np.zeros(len(rays), _abi.RADIANCE), np.zeros(len(rays), np.int32)
    rc = lib().emt_trace_counting_ties(C.c_void_p(session._ctx), C.c_int(len(rays)), _p(rays), C.c_int(n_samples), C.c_uint32(first_frame), _p(out), _p(ties))
    assert rc == 0, rc
    return out, ties
