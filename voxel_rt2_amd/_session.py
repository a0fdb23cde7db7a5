"""Thin ctypes session over a library exporting the include/vrt_api.h entry points.

In the product the only caller is renderer.Renderer, which passes libvrt_hip.so (loaded by
_lib.py, which raises if the HIP library is missing -- there is no CPU fallback).  The parity
tests reuse this class for the test oracle, whose C entry points have the same shapes.
"""
import ctypes as C
import numpy as np

from . import _abi


class NativeError(RuntimeError):
    pass


class NativeSession:
    def __init__(self, lib, prefix, cfg, create_extra=()):
        self._lib, self._p = lib, prefix
        _abi.declare(lib, prefix)
        create = getattr(lib, prefix + "create")
        create.restype = C.c_void_p
        self.cfg = cfg
        self.W, self.H = cfg.width, cfg.height
        self.rows = (cfg.row_begin, cfg.row_end) if cfg.row_end > cfg.row_begin else (0, cfg.height)
        self._ctx = create(C.byref(cfg), *create_extra)
        if not self._ctx:
            raise NativeError(f"{prefix}create failed: {self._err()}")

    def _err(self):
        fn = getattr(self._lib, self._p + "last_error", None)
        if fn is None:
            return "(no message)"
        msg = fn()
        return msg.decode() if msg else "(no message)"

    def _call(self, name, *args):
        if not self._ctx:
            raise NativeError("session is closed")
        rc = getattr(self._lib, self._p + name)(C.c_void_p(self._ctx), *args)
        if rc != 0:
            raise NativeError(f"{self._p}{name} failed ({rc}): {self._err()}")

    def close(self):
        """Ends the session.  Page-locked arrays from host_alloc() die with it (see there): outstanding asynchronous fetches are
        waited for first, so that no copy is still writing into memory that is being freed."""
        if self._ctx:
            pinned = getattr(self, "_pinned", [])
            if pinned:
                wait = getattr(self._lib, self._p + "fetch_wait", None)
                if wait is not None:
                    for slot in range(4):       # VRT_FETCH_SLOTS; a slot without a fetch returns at once
                        wait(C.c_void_p(self._ctx), slot)
                for ptr, _ in pinned:
                    getattr(self._lib, self._p + "host_free")(C.c_void_p(self._ctx), C.c_void_p(ptr))
            self._pinned = []
            getattr(self._lib, self._p + "destroy")(C.c_void_p(self._ctx))
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- uploads ---------------------------------------------------------------------------
    def upload_voxels(self, mat, rgb):
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        g = int(self.cfg.grid_res)
        if mat.shape != (g, g, g) or rgb.shape != (g, g, g, 3):
            raise ValueError(f"voxel arrays must be int8[{g},{g},{g}] and uint8[{g},{g},{g},3] (grid_res = {g})")
        self._call("upload_voxels", mat.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p))

    def update_voxels(self, lo, hi, mat, rgb, on_device=False):
        """Replace the voxels of the box [lo, hi) of a prepared scene (include/vrt_api.h, vrt_update_voxels).  Host path: `mat` and
        `rgb` are arrays of shape hi - lo and (hi - lo, 3).  Device path (on_device=True): they are integer device pointers to
        int8[hx][hy][hz] and uint8[hx][hy][hz][3] (a torch tensor's data_ptr()), read on the context's stream."""
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        if len(lo) != 3 or len(hi) != 3:
            raise ValueError("lo and hi are three coordinates each")
        if on_device:
            pm, pr = C.c_void_p(int(mat)), C.c_void_p(int(rgb))
        else:
            shape = tuple(max(h - l, 0) for l, h in zip(lo, hi))
            mat = np.ascontiguousarray(mat, dtype=np.int8)
            rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
            if mat.shape != shape or rgb.shape != shape + (3,):
                raise ValueError(f"box arrays must be int8{list(shape)} and uint8{list(shape + (3,))} for the box {lo}..{hi}")
            pm, pr = mat.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p)
        self._call("update_voxels", (C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi), pm, pr, int(bool(on_device)))

    def voxelize_triangles(self, tris, lo, hi, n=None):
        """Triangles voxelised into the box [lo, hi) of a prepared scene (include/vrt_api.h, vrt_voxelize_triangles).  Host path: `tris`
        is an array of _abi.TRIANGLE.  Device path: a torch tensor on the device holding the same 48-byte records (any dtype; `n`
        triangles, by default as many as it holds), read on the session's stream.  Returns the result record, a numpy scalar of
        _abi.VOXELIZE_RESULT (lo, hi, voxels, invalid)."""
        return self._triangles("voxelize_triangles", tris, lo, hi, n)

    def fill_triangles(self, tris, lo, hi, voxel, n=None):
        """The inside of a triangle mesh filled with the payload `voxel` (r | g << 8 | b << 16 | material byte << 24; material 0 carves)
        in the box [lo, hi) of a prepared scene (include/vrt_api.h, vrt_fill_triangles).  `tris`, `n` and the returned record are
        voxelize_triangles': host arrays of _abi.TRIANGLE or a device tensor of the same records, taken without a copy; the record
        counts and bounds the inside cells."""
        return self._triangles("fill_triangles", tris, lo, hi, n, C.c_uint32(int(voxel) & 0xFFFFFFFF))

    def _triangles(self, entry, tris, lo, hi, n, *extra):
        """The two triangle entry points' handling of their arrays; `extra`: arguments between the box and the result record."""
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        if len(lo) != 3 or len(hi) != 3:
            raise ValueError("lo and hi are three coordinates each")
        res = np.zeros(1, _abi.VOXELIZE_RESULT)
        size = _abi.TRIANGLE.itemsize
        if hasattr(tris, "data_ptr"):
            if not getattr(tris, "is_cuda", False):   # (a host tensor's address must never reach the kernels as a device pointer)
                raise ValueError("device path: the tensor must live on the device; hand host triangles over as a numpy array of _abi.TRIANGLE")
            count = tris.numel() * tris.element_size() // size if n is None else int(n)
            if count < 0 or tris.numel() * tris.element_size() < count * size or not tris.is_contiguous():
                raise ValueError(f"device path: {count} triangles are a contiguous device tensor of {count * size} bytes")
            ptr, on_device = C.c_void_p(tris.data_ptr()), 1
        else:
            tris = np.ascontiguousarray(tris, dtype=_abi.TRIANGLE).reshape(-1)
            count, ptr, on_device = len(tris), tris.ctypes.data_as(C.c_void_p), 0
        if count == 0:   # (an empty array's pointer may be NULL, which the library refuses whatever n is: it checks box and state all the same)
            none = np.zeros(1, _abi.TRIANGLE)
            ptr, on_device = none.ctypes.data_as(C.c_void_p), 0
        self._call(entry, C.c_int64(count), ptr, (C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi), *extra, res.ctypes.data_as(C.c_void_p), on_device)
        return res[0]

    def _query(self, entry, records, out, n, in_name, out_name, extra, noun, what):
        """The three scene queries' handling of their arrays: `records` of dtype _abi.<in_name> in, `out` of _abi.<out_name> back,
        `extra` arguments between them.  noun, what: the messages' words for an input record and for the results."""
        in_dtype, out_dtype = getattr(_abi, in_name), getattr(_abi, out_name)
        i, o = in_dtype.itemsize, out_dtype.itemsize
        if hasattr(records, "data_ptr"):
            if out is None or not hasattr(out, "data_ptr"):
                raise ValueError(f"device path: `out` is a device tensor of {o} bytes a {noun}")
            count = records.numel() * records.element_size() // i if n is None else int(n)
            if records.numel() * records.element_size() < count * i or out.numel() * out.element_size() < count * o:
                raise ValueError(f"{count} {noun}s need {count * i} bytes of {noun}s and {count * o} bytes of {what}")
            if not (records.is_contiguous() and out.is_contiguous()):
                raise ValueError("device tensors must be contiguous")
            self._call(entry, C.c_int64(count), C.c_void_p(records.data_ptr()), *extra, C.c_void_p(out.data_ptr()), 1)
            return out
        records = np.ascontiguousarray(records, dtype=in_dtype).reshape(-1)
        if out is None:
            out = np.empty(len(records), out_dtype)
        if out.dtype != out_dtype or out.shape != records.shape or not out.flags.c_contiguous:
            raise ValueError(f"`out` must be a contiguous array of _abi.{out_name}, one record a {noun}")
        if len(records):   # (an empty array's pointer may be NULL, which the library refuses whatever n is)
            self._call(entry, C.c_int64(len(records)), records.ctypes.data_as(C.c_void_p), *extra, out.ctypes.data_as(C.c_void_p), 0)
        return out

    def cast_rays(self, rays, out=None, n=None):
        """Rays against the prepared scene (include/vrt_api.h, vrt_cast_rays).  Host path: `rays` is an array of _abi.RAY, the result
        an array of _abi.HIT (`out` if given).  Device path: `rays` and `out` are torch tensors on the device holding the same 32-
        and 48-byte records (any dtype; `n` rays, by default as many as `rays` holds); the work is queued on the session's stream and
        `out` is returned, not yet filled."""
        return self._query("cast_rays", rays, out, n, "RAY", "HIT", (), "ray", "records")

    def sweep_boxes(self, boxes, out=None, n=None):
        """Moving boxes against the prepared scene (include/vrt_api.h, vrt_sweep_boxes).  Host path: `boxes` is an array of
        _abi.BOX_SWEEP, the result an array of _abi.SWEEP_HIT (`out` if given).  Device path: `boxes` and `out` are torch tensors on the
        device holding the same 48- and 32-byte records (any dtype; `n` boxes, by default as many as `boxes` holds); the work is queued
        on the session's stream and `out` is returned, not yet filled."""
        return self._query("sweep_boxes", boxes, out, n, "BOX_SWEEP", "SWEEP_HIT", (), "box", "records")

    def trace_radiance(self, rays, samples=1, first_frame=0, out=None, n=None):
        """Path-traced radiance along rays (include/vrt_api.h, vrt_trace_radiance): the mean of `samples` samples a ray, sample s on
        random stream (seed, first_frame + s, ray.stream, 0).  Host path: `rays` is an array of _abi.PATH_RAY, the result an array of
        _abi.RADIANCE (`out` if given).  Device path: `rays` and `out` are torch tensors on the device holding the same 32- and 16-byte
        records (any dtype; `n` rays, by default as many as `rays` holds); the work is queued on the session's stream and `out` is
        returned, not yet filled."""
        extra = (int(samples), C.c_uint32(int(first_frame) & 0xFFFFFFFF))
        return self._query("trace_radiance", rays, out, n, "PATH_RAY", "RADIANCE", extra, "ray", "results")

    def gather_irradiance(self, sensors, samples=1, first_frame=0, out=None, n=None):
        """Irradiance at surface points (include/vrt_api.h, vrt_gather_irradiance): per sensor the means over `samples` samples of the
        hemisphere's light, its open share, the sun's light and its visible share; sample s draws its directions from random stream
        (seed, first_frame + s, sensor.stream, 4).  Host path: `sensors` is an array of _abi.SENSOR, the result an array of
        _abi.IRRADIANCE (`out` if given).  Device path: `sensors` and `out` are torch tensors on the device holding the same 32-byte
        records (any dtype; `n` sensors, by default as many as `sensors` holds); the work is queued on the session's stream and `out`
        is returned, not yet filled."""
        extra = (int(samples), C.c_uint32(int(first_frame) & 0xFFFFFFFF))
        return self._query("gather_irradiance", sensors, out, n, "SENSOR", "IRRADIANCE", extra, "sensor", "results")

    def gather_probes(self, probes, samples=1, first_frame=0, out=None, n=None):
        """Spherical-harmonic light probes at points in empty space (include/vrt_api.h, vrt_gather_probes): per probe the means over
        `samples` samples of nine coefficients per colour channel of the arriving radiance, the open share of the sphere, the sun's
        light on a surface that faces it and the visible share of its disc; sample s draws its directions from random stream
        (seed, first_frame + s, probe.stream, 5).  Host path: `probes` is an array of _abi.PROBE, the result an array of
        _abi.SH_PROBE (`out` if given).  Device path: `probes` and `out` are torch tensors on the device holding the same 16- and
        128-byte records (any dtype; `n` probes, by default as many as `probes` holds); the work is queued on the session's stream and
        `out` is returned, not yet filled."""
        extra = (int(samples), C.c_uint32(int(first_frame) & 0xFFFFFFFF))
        return self._query("gather_probes", probes, out, n, "PROBE", "SH_PROBE", extra, "probe", "results")

    def fetch_voxels(self, lo, hi, mat=None, rgb=None, on_device=False):
        """The stored voxels of the box [lo, hi) (include/vrt_api.h, vrt_fetch_voxels).  Host path: returns (mat, rgb), arrays of shape
        hi - lo and (hi - lo, 3).  Device path (on_device=True): `mat` and `rgb` are integer device pointers to int8[hx][hy][hz] and
        uint8[hx][hy][hz][3], written on the session's stream."""
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        if len(lo) != 3 or len(hi) != 3:
            raise ValueError("lo and hi are three coordinates each")
        if on_device:
            self._call("fetch_voxels", (C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi), C.c_void_p(int(mat)), C.c_void_p(int(rgb)), 1)
            return None
        shape = tuple(max(h - l, 0) for l, h in zip(lo, hi))
        mat, rgb = np.zeros(shape, np.int8), np.zeros(shape + (3,), np.uint8)
        if mat.size:   # (an empty box copies nothing, and an empty array's pointer may be NULL, which the library refuses)
            self._call("fetch_voxels", (C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi), mat.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p), 0)
        return mat, rgb

    def distance_field(self, lo, hi, max_d2=None, to_empty=False, nearest=False, out=None):
        """The exact squared distance from every cell of the box [lo, hi) to the nearest solid voxel of the grid (to_empty: to the
        nearest non-solid cell), and with nearest=True that voxel's linear index (include/vrt_api.h, vrt_distance_field).  max_d2:
        distances beyond it are _abi.DIST_FAR (nearest -1); None: unbounded.  Host path: returns d2, or (d2, nearest), int32 arrays of
        shape hi - lo; `out`, if given, is that array or pair, filled in place.  Device path: `out` is a torch int32 tensor on the
        device of that shape, or a pair of them with nearest=True, taken without a copy; the work is queued on the session's stream and
        `out` is returned, not yet filled."""
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        if len(lo) != 3 or len(hi) != 3:
            raise ValueError("lo and hi are three coordinates each")
        shape = tuple(max(h - l, 0) for l, h in zip(lo, hi))
        max_d2 = _abi.DIST_MAX_D2 if max_d2 is None else int(max_d2)
        flags = C.c_uint32(_abi.DIST_TO_EMPTY if to_empty else 0)
        parts = (out if nearest else (out,)) if out is not None else None
        if parts is not None and len(parts) != (2 if nearest else 1):
            raise ValueError("`out` is one array, or the pair (d2, nearest) with nearest=True")
        if parts is not None and hasattr(parts[0], "data_ptr"):
            import torch
            for t in parts:
                if not hasattr(t, "data_ptr") or t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
                    raise ValueError(f"device path: `out` holds contiguous int32 device tensors of shape {list(shape)}")
            if parts[0].numel():   # (an empty tensor's pointer may be NULL, which the library refuses; it checks box and state all the same)
                ptrs = [C.c_void_p(t.data_ptr()) for t in parts] + [None] * (2 - len(parts))
                self._call("distance_field", (C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi), max_d2, flags, ptrs[0], ptrs[1], 1)
            else:
                none = np.zeros(1, np.int32)
                self._call("distance_field", (C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi), max_d2, flags, none.ctypes.data_as(C.c_void_p), None, 0)
            return out
        if parts is None:
            parts = tuple(np.empty(shape, np.int32) for _ in range(2 if nearest else 1))
        for a in parts:
            if not isinstance(a, np.ndarray) or a.dtype != np.int32 or a.shape != shape or not a.flags.c_contiguous:
                raise ValueError(f"`out` holds contiguous int32 arrays of shape {list(shape)}")
        ptrs = [a.ctypes.data_as(C.c_void_p) for a in parts] + [None] * (2 - len(parts))
        if parts[0].size == 0:   # (as above)
            ptrs[0], ptrs[1] = np.zeros(1, np.int32).ctypes.data_as(C.c_void_p), None
        self._call("distance_field", (C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi), max_d2, flags, ptrs[0], ptrs[1], 0)
        return parts if nearest else parts[0]

    def label_components(self, lo, hi, connectivity=6, empty=False, out=None):
        """The connected components of the solid cells of the box [lo, hi) (empty: of its non-solid cells) under 6-, 18- or
        26-connectivity: every member labelled with the smallest linear grid index of its component, every other cell -1
        (include/vrt_api.h, vrt_label_components).  Cells outside the box do not exist.  Host path: returns (labels, result) -- an
        int32 array of shape hi - lo (`out` if given, filled in place) and the dict of cells, components, reserved.  Device path:
        `out` is a torch int32 tensor on the device of that shape, or the pair (labels, result) with `result` a device tensor of 16
        bytes (_abi.LABEL_RESULT), taken without a copy; the work is queued on the session's stream and `out` is returned, not yet
        filled."""
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        if len(lo) != 3 or len(hi) != 3:
            raise ValueError("lo and hi are three coordinates each")
        if connectivity not in (6, 18, 26):
            raise ValueError("connectivity is 6, 18 or 26")
        shape = tuple(max(h - l, 0) for l, h in zip(lo, hi))
        flags = C.c_uint32({6: 0, 18: _abi.LABEL_CONN_18, 26: _abi.LABEL_CONN_26}[connectivity] | (_abi.LABEL_EMPTY if empty else 0))
        box = ((C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi))
        labels, result = out if isinstance(out, (tuple, list)) else (out, None)
        if hasattr(labels, "data_ptr"):
            import torch
            if labels.dtype != torch.int32 or tuple(labels.shape) != shape or not labels.is_contiguous():
                raise ValueError(f"device path: the labels are a contiguous int32 device tensor of shape {list(shape)}")
            if result is not None and (not hasattr(result, "data_ptr") or result.numel() * result.element_size() != 16 or not result.is_contiguous()):
                raise ValueError("device path: `result` is a contiguous device tensor of 16 bytes")
            res = C.c_void_p(result.data_ptr()) if result is not None else None
            if labels.numel():   # (an empty tensor's pointer may be NULL, which the library refuses; it checks box and state all the same)
                self._call("label_components", *box, flags, C.c_void_p(labels.data_ptr()), res, 1)
            else:
                self._call("label_components", *box, flags, C.c_void_p(result.data_ptr()) if result is not None else np.zeros(1, np.int32).ctypes.data_as(C.c_void_p), res,
                           1 if result is not None else 0)
            return out
        if result is not None:
            raise ValueError("host path: `out` is the labels array; the result record is returned")
        if labels is None:
            labels = np.empty(shape, np.int32)
        if not isinstance(labels, np.ndarray) or labels.dtype != np.int32 or labels.shape != shape or not labels.flags.c_contiguous:
            raise ValueError(f"`out` is a contiguous int32 array of shape {list(shape)}")
        rec = np.zeros(1, _abi.LABEL_RESULT)
        ptr = labels.ctypes.data_as(C.c_void_p) if labels.size else np.zeros(1, np.int32).ctypes.data_as(C.c_void_p)   # (as above)
        self._call("label_components", *box, flags, ptr, rec.ctypes.data_as(C.c_void_p), 0)
        return labels, {k: int(rec[0][k]) for k in ("cells", "components", "reserved")}

    def move_voxels(self, src_lo, src_hi, dst_lo, dst_hi, m, t, flags=0, select=None, select_value=0):
        """Move or copy the piece cells of the source box [src_lo, src_hi) into the destination box [dst_lo, dst_hi) under the integer
        map (m: nine Q16 coefficients, row-major; t: three offsets in 2^-17 voxels) from destination cell to source cell
        (include/vrt_api.h, vrt_move_voxels).  flags: _abi.MOVE_*.  select: None, a contiguous int32 array of the source box's shape
        (host path: staged by the call) or a contiguous int32 torch tensor on the device of that shape, read in place without a
        copy; a source cell takes part iff its entry equals select_value.  Returns the dict of lo, hi, written, blocked, erased; the
        call has waited for the device."""
        rec = np.zeros(1, _abi.VOXEL_MOVE)
        for name, v in (("src_lo", src_lo), ("src_hi", src_hi), ("dst_lo", dst_lo), ("dst_hi", dst_hi), ("t", t)):
            v = [int(x) for x in v]
            if len(v) != 3:
                raise ValueError(f"{name} has three entries")
            if name == "t" and any(abs(x) >= 1 << 63 for x in v):
                raise ValueError("t does not fit 64 bits")
            rec[0][name] = v
        m = [int(x) for x in np.asarray(m, dtype=object).reshape(-1)]
        if len(m) != 9 or any(abs(x) >= 1 << 31 for x in m):
            raise ValueError("m has nine entries that fit 32 bits")
        rec[0]["m"], rec[0]["select_value"], rec[0]["flags"] = m, int(select_value), int(flags)
        shape = tuple(max(int(h) - int(l), 0) for l, h in zip(src_lo, src_hi))
        ptr, on_device = None, 0
        if select is not None and hasattr(select, "data_ptr"):
            import torch
            if select.dtype != torch.int32 or tuple(select.shape) != shape or not select.is_contiguous():
                raise ValueError(f"device path: `select` is a contiguous int32 device tensor of shape {list(shape)}")
            ptr, on_device = (C.c_void_p(select.data_ptr()) if select.numel() else None), 1
        elif select is not None:
            if not isinstance(select, np.ndarray) or select.dtype != np.int32 or select.shape != shape or not select.flags.c_contiguous:
                raise ValueError(f"`select` is a contiguous int32 array of shape {list(shape)}")
            ptr = select.ctypes.data_as(C.c_void_p) if select.size else None
        res = np.zeros(1, _abi.MOVE_RESULT)
        self._call("move_voxels", rec.ctypes.data_as(C.c_void_p), ptr, on_device, res.ctypes.data_as(C.c_void_p))
        return dict(lo=tuple(int(v) for v in res[0]["lo"]), hi=tuple(int(v) for v in res[0]["hi"]), written=int(res[0]["written"]),
                    blocked=int(res[0]["blocked"]), erased=int(res[0]["erased"]))

    def upload_materials(self, table):
        table = np.ascontiguousarray(table, dtype=np.float32)
        if table.shape != (128, 14):
            raise ValueError("material table must be float32[128,14]")
        self._call("upload_materials", table.ctypes.data_as(C.c_void_p))

    def upload_cloud_texture(self, tex):
        tex = np.ascontiguousarray(tex, dtype=np.uint8)
        if tex.shape != (256, 256, 3):
            raise ValueError("cloud texture must be uint8[256,256,3]")
        self._call("upload_cloud_texture", tex.ctypes.data_as(C.c_void_p))

    def set_scene(self, scene):
        self._call("set_scene", C.byref(scene))

    def set_camera(self, cam):
        self._call("set_camera", C.byref(cam))

    def set_reference_indexing(self, on=True):
        """Occupancy queries outside the grid read the bit the reference's own index arithmetic addresses (raytracer.py:17-44)
        instead of "empty": include/vrt_api.h, vrt_set_reference_indexing."""
        self._call("set_reference_indexing", int(bool(on)))

    def set_row_stripes(self, stripe_rows, n_parts, part):
        """This (whole-frame) context produces every n_parts-th stripe of stripe_rows rows: include/vrt_api.h, vrt_set_row_stripes."""
        self._call("set_row_stripes", int(stripe_rows), int(n_parts), int(part))
        self.stripes = (int(stripe_rows), int(n_parts), int(part)) if stripe_rows else None

    @property
    def io_on_device(self):
        """Whether the *_io entry points take device memory (the HIP library) or host memory (the oracle)."""
        return self._p == "vrt_"

    def set_history_exchange(self, on=True):
        """Row tile: keep the previous frame's temporal state of the whole frame, so that the moving camera can run on it
        (include/vrt_api.h, vrt_set_history_exchange; parallel.exchange_history moves the rows between ranks)."""
        self._call("set_history_exchange", int(bool(on)))

    def history_rows_io(self, row0, row1, ptr, to_library):
        """Rows [row0, row1) of the temporal state <-> device memory at `ptr`: four planes back to back, 40 bytes a pixel
        (include/vrt_api.h, vrt_history_rows_io).  to_library False exports own rows, True imports other rows."""
        self._call("history_rows_io", int(row0), int(row1), C.c_void_p(int(ptr)), int(bool(to_library)))

    def owned_rows(self):
        """Row indices this session produces, in the order its device tiles hold them."""
        st = getattr(self, "stripes", None)
        if not st:
            return np.arange(self.rows[0], self.rows[1])
        s_, n_, p_ = st
        return np.concatenate([np.arange(a, min(a + s_, self.H)) for a in range(p_ * s_, self.H, s_ * n_)])

    # -- work ------------------------------------------------------------------------------
    def prepare(self):
        self._call("prepare")

    def sky_accumulate_clouds(self, max_samples):
        self._call("sky_accumulate_clouds", int(max_samples))

    def sky_compute_slice(self, slice_idx, max_slices):
        self._call("sky_compute_slice", int(slice_idx), int(max_slices))

    def sky_accumulate_clouds_slice(self, max_samples, slice_idx, max_slices):
        self._call("sky_accumulate_clouds_slice", int(max_samples), int(slice_idx), int(max_slices))

    def sky_table_io(self, which, u0, u1, ptr, to_library):
        """Columns [u0, u1) of a sky table <-> caller memory at `ptr` (device memory for the HIP library, host for the oracle)."""
        self._call("sky_table_io", int(which), int(u0), int(u1), C.c_void_p(int(ptr)), int(bool(to_library)))

    def accumulate(self, n=1):
        self._call("accumulate", int(n))

    def reset(self):
        self._call("reset")

    def end_frame(self):
        self._call("end_frame")

    def sync(self):
        if getattr(self._lib, self._p + "sync", None) is not None:
            self._call("sync")

    # -- results ---------------------------------------------------------------------------
    def fetch_hdr(self):
        out = np.empty((self.H, self.W, 3), dtype=np.float32)
        self._call("fetch_hdr", out.ctypes.data_as(C.c_void_p))
        return out

    def fetch_hdr_device(self, device_ptr):
        self._call("fetch_hdr_device", C.c_void_p(int(device_ptr)))

    def fetch_hdr_device_async(self, device_ptr):
        self._call("fetch_hdr_device_async", C.c_void_p(int(device_ptr)))

    def reserve_cus(self, n_cus):
        """Leave n_cus CUs' worth of workgroup slots out of the persistent render grid (multi-GPU: room for RCCL's kernels)."""
        if getattr(self._lib, self._p + "reserve_cus", None) is not None:
            self._call("reserve_cus", int(n_cus))

    def set_stream(self, hip_stream):
        self._call("set_stream", C.c_void_p(int(hip_stream) if hip_stream else None))

    def fetch_ldr(self):
        out = np.empty((self.H, self.W, 4), dtype=np.float32)
        self._call("fetch_ldr", out.ctypes.data_as(C.c_void_p))
        return out

    # -- presenting every frame (the reference's accumulate / fetch_image / copy_prev_matrices loop, scene.py:255-262) ---
    def host_alloc(self, shape, dtype=np.float32):
        """Page-locked host array (vrt_host_alloc): the target of the asynchronous fetches.  The memory belongs to the SESSION:
        close() frees it, after which the array must not be touched -- copy what has to outlive the session
        (Renderer.present_wait returns copies)."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = C.c_void_p()
        self._call("host_alloc", C.c_uint64(n), C.byref(ptr))
        buf = (C.c_char * n).from_address(ptr.value)
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append((ptr.value, arr))
        return arr

    def fetch_hdr_async(self, out, slot=0):
        assert out.dtype == np.float32 and out.shape == (self.H, self.W, 3) and out.flags.c_contiguous
        self._call("fetch_hdr_async", out.ctypes.data_as(C.c_void_p), int(slot))

    def fetch_ldr_async(self, out, slot=0):
        assert out.dtype == np.float32 and out.shape == (self.H, self.W, 4) and out.flags.c_contiguous
        self._call("fetch_ldr_async", out.ctypes.data_as(C.c_void_p), int(slot))

    def fetch_ldr8_async(self, out, slot=0):
        assert out.dtype == np.uint8 and out.shape == (self.H, self.W, 4) and out.flags.c_contiguous
        self._call("fetch_ldr8_async", out.ctypes.data_as(C.c_void_p), int(slot))

    def fetch_wait(self, slot=0):
        self._call("fetch_wait", int(slot))

    # -- multi-GPU hand-over: the temporal pass writes the rank's HDR tile itself (vrt_set_hdr_targets) ---------------
    def set_hdr_targets(self, device_ptrs):
        arr = (C.c_void_p * len(device_ptrs))(*[int(p) for p in device_ptrs])
        self._call("set_hdr_targets", arr, len(device_ptrs))

    def hdr_targets_written(self):
        n = C.c_uint64(0)
        self._call("hdr_targets_written", C.byref(n))
        return int(n.value)

    _BUF = {
        _abi.BUF_GBUF_DEPTH: (np.float32, 1), _abi.BUF_GBUF_NORMAL: (np.uint16, 2), _abi.BUF_GBUF_POSITION: (np.float32, 3),
        _abi.BUF_GBUF_MAT: (np.uint32, 1), _abi.BUF_GBUF_REFL_DEPTH: (np.float32, 1),
        _abi.BUF_HISTORY_DIFFUSE: (np.float32, 4), _abi.BUF_HISTORY_SPECULAR: (np.float32, 4),
    }

    def fetch_buffer(self, which):
        if which in self._BUF:
            dt, k = self._BUF[which]
            out = np.empty((self.H, self.W, k), dtype=dt)
        elif which in (_abi.BUF_SKY_SCATTERING, _abi.BUF_SKY_TRANSMITTANCE):
            r = self.cfg.sky_res
            out = np.empty((r, r, 3), dtype=np.float32)
        elif which == _abi.BUF_TRANS_LUT:
            out = np.empty((256, 128, 3), dtype=np.uint16)
        else:
            raise ValueError(f"unknown buffer id {which}")
        self._call("fetch_buffer", int(which), out.ctypes.data_as(C.c_void_p))
        return out

    def denoise(self, params=None, out=None):
        """The accumulated frame through the g-buffer-guided a-trous filter (include/vrt_api.h, vrt_denoise): HDR float32[H][W][3].
        `params` is an _abi.VrtDenoiseParams (None: the library's defaults).  Host path: the result is an array (`out` if given).  Device
        path: `out` is a torch tensor on the device of H * W * 12 bytes; the work is queued on the session's stream and `out` is returned,
        not yet filled."""
        p = None if params is None else C.byref(params)
        if out is not None and hasattr(out, "data_ptr"):
            if out.numel() * out.element_size() < self.H * self.W * 12 or not out.is_contiguous():
                raise ValueError(f"device path: `out` is a contiguous device tensor of {self.H * self.W * 12} bytes")
            self._call("denoise", p, C.c_void_p(out.data_ptr()), 1)
            return out
        if out is None:
            out = np.empty((self.H, self.W, 3), dtype=np.float32)
        if out.dtype != np.float32 or out.shape != (self.H, self.W, 3) or not out.flags.c_contiguous:
            raise ValueError("`out` must be a contiguous float32 array [H, W, 3]")
        self._call("denoise", p, out.ctypes.data_as(C.c_void_p), 0)
        return out

    def stats(self):
        s = _abi.VrtStats()
        self._call("get_stats", C.byref(s))
        return s.as_dict()
