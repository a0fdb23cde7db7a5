"""`Renderer`: the drop-in for the reference's renderer.pathtracer.Renderer, on libvrt_hip.so.

Same constructor and method names as /root/reference/renderer/pathtracer.py (the surface that
scene.py drives); every method forwards to the C ABI of include/vrt_api.h.
Scalar fields the reference pokes with ``field[None] = x`` (floor_height, floor_color,
floor_material, background_color, use_physical_atmosphere, atmos.use_clouds, fov) are `_Field`
objects supporting the same syntax.  The module constants of the reference are keyword arguments
/ environment variables here: VRT_MAX_DEPTH (MAX_RAY_DEPTH, default 4), VRT_RESTIR (USE_RESTIR_PT,
default 0), VRT_SEED, VRT_SKY_RES (default 3840).
"""
import ctypes as C
import math
import os
import struct
import numpy as np

from . import _abi, _lib, camera as cam_mod, host, materials
from ._session import NativeSession, NativeError  # noqa: F401


class _Field:
    """Stand-in for a 0-d Taichi field: ``f[None] = v`` / ``f[None]``."""

    def __init__(self, value, on_change=None):
        self._v, self._cb = value, on_change

    def __getitem__(self, _):
        return self._v

    def __setitem__(self, _, value):
        self._v = value
        if self._cb:
            self._cb()


class _AtmosProxy:
    def __init__(self, on_change):
        self.use_clouds = _Field(0, on_change)


_F32 = struct.Struct("f")


def _f32(x):
    """x rounded to binary32 (the reference's voxel colours are f32 vectors)."""
    return _F32.unpack(_F32.pack(x))[0]


class VoxelStore:
    """Renderer.set_voxel / get_voxel and their storage (pathtracer.py:1325-1334, voxel_world.py:7-18):
    int8 material + uint8 rgb per voxel, index (x+G/2, y+G/2, z+G/2), G = voxel_grid_res (128 in the reference,
    pathtracer.py:83).  Kept on the host because the example kernels author the scene on the host; bytearray-backed
    so a per-voxel call costs ~1 us."""

    def _init_voxels(self, grid_res=128):
        g = self.voxel_grid_res = int(grid_res)
        self._mat = bytearray(g * g * g)
        self._rgb = bytearray(g * g * g * 3)
        self.voxel_material = np.frombuffer(self._mat, dtype=np.int8).reshape(g, g, g)
        self.voxel_color = np.frombuffer(self._rgb, dtype=np.uint8).reshape(g, g, g, 3)
        self._voxels_dirty = True
        self._dirty_lo, self._dirty_hi = [0, 0, 0], [g, g, g]   # bounding box of the voxels written since the last upload

    def set_voxel(self, idx, mat, color):
        g = self.voxel_grid_res
        h = g >> 1
        x, y, z = int(idx[0]) + h, int(idx[1]) + h, int(idx[2]) + h
        if not (0 <= x < g and 0 <= y < g and 0 <= z < g):
            return  # the reference writes out of bounds here (undefined behaviour)
        i = (x * g + y) * g + z
        self._mat[i] = int(mat) & 0xFF  # ti.cast(mat, ti.i8)
        rgb = self._rgb
        j = 3 * i
        for k in (0, 1, 2):  # math_utils.py:86-92: u8(clamp(c, 0, 1) * 255), evaluated in f32
            c = _f32(color[k])
            c = 0.0 if c < 0.0 else (1.0 if c > 1.0 else c)
            rgb[j + k] = int(_f32(c * 255.0))
        self._voxels_dirty = True
        lo, hi = self._dirty_lo, self._dirty_hi
        if lo[0] >= hi[0]:   # nothing written since the last upload
            lo[:], hi[:] = (x, y, z), (x + 1, y + 1, z + 1)
        else:
            for a, v in enumerate((x, y, z)):
                if v < lo[a]:
                    lo[a] = v
                if v >= hi[a]:
                    hi[a] = v + 1

    def get_voxel(self, ijk):
        g = self.voxel_grid_res
        h = g >> 1
        x, y, z = int(ijk[0]) + h, int(ijk[1]) + h, int(ijk[2]) + h
        if not (0 <= x < g and 0 <= y < g and 0 <= z < g):
            return 0, (0.0, 0.0, 0.0)
        i = (x * g + y) * g + z
        m = self._mat[i]
        j = 3 * i
        return (m - 256 if m > 127 else m), (_f32(self._rgb[j] / 255.0), _f32(self._rgb[j + 1] / 255.0), _f32(self._rgb[j + 2] / 255.0))

    def set_voxel_arrays(self, mat, rgb):
        self.voxel_material[...] = mat
        self.voxel_color[...] = rgb
        self._voxels_dirty = True
        g = self.voxel_grid_res
        self._dirty_lo, self._dirty_hi = [0, 0, 0], [g, g, g]

    def dirty_box(self):
        """(lo, hi): bounding box [lo, hi) of the voxels written since the last upload, in array indices; lo == hi: none."""
        return tuple(self._dirty_lo), tuple(self._dirty_hi)

    def _voxels_uploaded(self):
        self._voxels_dirty = False
        self._dirty_lo, self._dirty_hi = [0, 0, 0], [0, 0, 0]

    # face k of a voxel: 0..5 = -x, +x, -y, +y, -z, +z
    FACE_NORMALS = np.array([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)], np.float32)

    def surface_faces(self, lo=None, hi=None):
        """The exposed faces of the solid voxels (material > 0) in the box [lo, hi) of array indices -- by default the whole grid: every
        face whose neighbour cell is empty or lies outside the grid.  Host numpy on voxel_material (after device-side edits run
        sync_voxels_from_device first).  Returns (cell int32[m, 3] array indices, face int8[m] 0..5 = -x, +x, -y, +y, -z, +z,
        centre float32[m, 3] the face's centre in world units, normal float32[m, 3]), faces in the order of `face`, then of the cells."""
        g = self.voxel_grid_res
        lo = np.clip(np.array((0, 0, 0) if lo is None else lo, np.int64), 0, g)
        hi = np.clip(np.array((g, g, g) if hi is None else hi, np.int64), 0, g)
        hi = np.maximum(hi, lo)
        pad = np.zeros((g + 2,) * 3, bool)
        pad[1:-1, 1:-1, 1:-1] = self.voxel_material > 0
        box = tuple(slice(int(a) + 1, int(b) + 1) for a, b in zip(lo, hi))
        solid = pad[box]
        cells, faces = [], []
        for k in range(6):                                      # six shifted comparisons
            axis, step = k >> 1, (k & 1) * 2 - 1
            there = tuple(slice(sl.start + step, sl.stop + step) if a == axis else sl for a, sl in enumerate(box))
            idx = np.argwhere(solid & ~pad[there])
            cells.append(idx + lo)
            faces.append(np.full(len(idx), k, np.int8))
        cell = np.concatenate(cells).astype(np.int32).reshape(-1, 3)
        face = np.concatenate(faces)
        normal = self.FACE_NORMALS[face]
        dx = 2.0 / g                                            # a cell spans [(i - g / 2) dx, (i + 1 - g / 2) dx]: exact in binary32
        centre = ((cell.astype(np.float64) + 0.5 - g / 2) * dx + normal.astype(np.float64) * (0.5 * dx)).astype(np.float32)
        return cell, face, centre, normal

    def probe_lattice(self, lo=None, hi=None, step=4):
        """Where light probes go: the EMPTY cells (material <= 0) of the box [lo, hi) of array indices -- by default the whole grid --
        taken every `step` cells from lo on each axis.  Host numpy on voxel_material, no device (after device-side edits run
        sync_voxels_from_device first).  Returns (centre float32[m, 3] the cells' centres in world units, cell int32[m, 3] array
        indices), x slowest."""
        g = self.voxel_grid_res
        step = int(step)
        if step < 1:
            raise ValueError("step must be at least 1")
        lo = np.clip(np.array((0, 0, 0) if lo is None else lo, np.int64), 0, g)
        hi = np.clip(np.array((g, g, g) if hi is None else hi, np.int64), 0, g)
        hi = np.maximum(hi, lo)
        axes = [np.arange(int(a), int(b), step) for a, b in zip(lo, hi)]
        cell = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
        cell = cell[self.voxel_material[cell[:, 0], cell[:, 1], cell[:, 2]] <= 0].astype(np.int32).reshape(-1, 3)
        centre = ((cell.astype(np.float64) + 0.5 - g / 2) * (2.0 / g)).astype(np.float32)
        return centre, cell

    # -- reading vrt_sh_probe records (include/vrt_api.h, vrt_gather_probes) ------------------------------------------------------
    SH_BAND_WEIGHTS = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)   # A_l per coefficient: the clamped-cosine lobe's

    @staticmethod
    def sh_basis(dirs):
        """Y0 .. Y8 of include/vrt_api.h at unit vectors: float64[n, 9], with the constants at float64's precision (the library's are
        their binary32 roundings).  The polar axis is z; the world's up is y."""
        d = np.asarray(dirs, np.float64).reshape(-1, 3)
        x, y, z = d[:, 0], d[:, 1], d[:, 2]
        k0, k1, k2, k3, k4 = 0.5 * np.sqrt(1.0 / np.pi), np.sqrt(0.75 / np.pi), 0.5 * np.sqrt(15.0 / np.pi), 0.25 * np.sqrt(5.0 / np.pi), 0.25 * np.sqrt(15.0 / np.pi)
        return np.stack([np.full(len(d), k0), k1 * y, k1 * z, k1 * x, k2 * (x * y), k2 * (y * z), k3 * (3.0 * (z * z) - 1.0), k2 * (x * z), k4 * (x * x - y * y)],
                        axis=1)

    @staticmethod
    def sh_radiance(records, dirs):
        """The plain expansion L(d) = sum_i sh[i] * Yi(d) of _abi.SH_PROBE records at unit directions: float64[n, 3].  records and dirs
        pair up one to one (one of either serves all of the other)."""
        sh = np.asarray(np.atleast_1d(records)["sh"], np.float64).reshape(-1, 9, 3)
        return (VoxelStore.sh_basis(dirs)[:, :, None] * sh).sum(axis=1)

    @staticmethod
    def sh_irradiance(records, normals, light_direction=None):
        """The irradiance on unit normals from _abi.SH_PROBE records, float64[n, 3]:
        E = pi c0 Y0 + (2 pi / 3) sum_{i=1..3} ci Yi(n) + (pi / 4) sum_{i=4..8} ci Yi(n) + sun_rgb * max(0, n . light_direction);
        the sun's term is left out when no light direction is passed.  records and normals pair up one to one (one of either serves
        all of the other)."""
        rec = np.atleast_1d(records)
        sh = np.asarray(rec["sh"], np.float64).reshape(-1, 9, 3)
        n = np.asarray(normals, np.float64).reshape(-1, 3)
        e = ((VoxelStore.sh_basis(n) * VoxelStore.SH_BAND_WEIGHTS)[:, :, None] * sh).sum(axis=1)
        if light_direction is not None:
            ndl = np.maximum(n @ np.asarray(light_direction, np.float64).reshape(3), 0.0)
            e = e + np.asarray(rec["sun_rgb"], np.float64).reshape(-1, 3) * ndl[:, None]
        return e


class Renderer(VoxelStore):
    def __init__(self, dx, image_res, up, voxel_edges, exposure=3, *, max_depth=None, use_restir=None, seed=None, sky_res=None,
                 device=0, rows=None, grid_res=None):
        self.image_res = tuple(int(x) for x in image_res)
        self.aspect_ratio = self.image_res[0] / self.image_res[1]
        self.exposure = exposure
        self.up = tuple(up)
        self.max_depth = int(os.environ.get("VRT_MAX_DEPTH", 4)) if max_depth is None else int(max_depth)
        self.use_restir = bool(int(os.environ.get("VRT_RESTIR", 0))) if use_restir is None else bool(use_restir)
        self.seed = int(os.environ.get("VRT_SEED", 0)) if seed is None else int(seed)
        self.sky_res = int(os.environ.get("VRT_SKY_RES", 3840)) if sky_res is None else int(sky_res)
        cfg = host.make_config(self.image_res[0], self.image_res[1], voxel_edges=voxel_edges, exposure=exposure,
                               max_depth=self.max_depth, use_restir=self.use_restir, seed=self.seed, sky_res=self.sky_res,
                               device=device, rows=rows, dx=dx,
                               grid_res=int(os.environ.get("VRT_GRID_RES", 128)) if grid_res is None else int(grid_res))
        self._s = NativeSession(_lib.load(), "vrt_", cfg)   # the library insists on dx == 2 / grid_res
        if int(os.environ.get("VRT_REFERENCE_INDEXING", 0)):
            self._s.set_reference_indexing(True)

        # voxel storage the user kernels write through set_voxel (voxel_world.py:7-18)
        self._init_voxels(cfg.grid_res)

        dirty = self._mark_scene_dirty
        self.floor_height = _Field(0.0, dirty)       # pathtracer.py:91-93
        self.floor_color = _Field((1.0, 1.0, 1.0), dirty)
        self.floor_material = _Field(1, dirty)
        self.background_color = _Field((0.0, 0.0, 0.0), dirty)
        self.use_physical_atmosphere = _Field(0, dirty)
        self.atmos = _AtmosProxy(dirty)
        self.fov = _Field(float(np.deg2rad(50.0)))    # pathtracer.py:89
        self._light = dict(direction=(1.0, 1.0, 1.0), cone=0.1, color=(0.0, 0.0, 0.0), weight=0.0)
        self._scene_dirty = True

        self._pos = cam_mod.DEFAULT_POS
        self._look_at = cam_mod.DEFAULT_LOOK_AT
        self._view = self._proj = None
        self._jitter_index = 0
        self._moving = False
        self._render_scale = 1.0
        self._max_samples = 999999999.0
        self._cam_dirty = True
        self.current_spp = 0
        self.current_frame = 0
        self._s.upload_materials(materials.load_table())
        if self.sky_res > 0:
            self._s.upload_cloud_texture(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "cloud_texture.npy")))

    # -- scalar state -----------------------------------------------------------------------
    def _mark_scene_dirty(self):
        self._scene_dirty = True

    def set_directional_light(self, direction, light_cone_angle, light_color):  # pathtracer.py:139-144
        self._light = dict(direction=tuple(direction), cone=float(light_cone_angle), color=tuple(light_color), weight=3.0)
        self._scene_dirty = True

    def set_camera_is_moving(self, val):
        self._moving, self._cam_dirty = bool(val), True

    def set_render_scale(self, val):
        self._render_scale, self._cam_dirty = float(val), True

    def set_max_samples(self, max_samples):
        self._max_samples, self._cam_dirty = float(max_samples), True

    def set_camera_pos(self, x, y, z):
        self._pos, self._cam_dirty = (float(x), float(y), float(z)), True

    def set_look_at(self, x, y, z):
        self._look_at = (float(x), float(y), float(z))

    def set_up(self, x, y, z):
        self.up = (float(x), float(y), float(z))

    def set_fov(self, fov):
        self.fov[None] = float(fov)

    def set_proj_mat(self, M):  # M in glm memory order, like ti.ui.Camera.get_projection_matrix
        self._proj = cam_mod.from_glm_memory(M)
        self._jitter_index += 1  # one TAA jitter draw per call (pathtracer.py:264-265)
        self._cam_dirty = True

    def set_view_mat(self, M):
        self._view = cam_mod.from_glm_memory(M)
        self._cam_dirty = True

    def copy_prev_matrices(self):
        self._push()
        self._s.end_frame()

    # -- state push -------------------------------------------------------------------------
    def _push(self):
        if self._scene_dirty:
            self._s.set_scene(host.make_scene_params(
                floor_height=self.floor_height[None], floor_color=self.floor_color[None], floor_material=self.floor_material[None],
                background_color=self.background_color[None], light_direction=self._light["direction"],
                light_cone=self._light["cone"], light_color=self._light["color"], light_weight=self._light["weight"],
                use_physical_sky=self.use_physical_atmosphere[None], use_clouds=self.atmos.use_clouds[None]))
            self._scene_dirty = False
        if self._cam_dirty:
            if self._view is None or self._proj is None:
                self._view, self._proj = cam_mod.default_matrices(*self.image_res, pos=self._pos, look=self._look_at, fov=self.fov[None])
            self._s.set_camera(host.make_camera(self._view, self._proj, self._pos, jitter_index=self._jitter_index,
                                                moving=self._moving, render_scale=self._render_scale,
                                                max_accum_frames=self._max_samples))
            self._cam_dirty = False

    # -- work (pathtracer.py:314-329, 664-668, 1310-1323) -------------------------------------
    def prepare_data(self):
        self._push()
        if self._voxels_dirty:
            self._s.upload_voxels(self.voxel_material, self.voxel_color)
            self._voxels_uploaded()
        self._s.prepare()
        self._prepared = True

    def update_voxels(self, reset=True):
        """Send the voxels written since the last upload (set_voxel, set_voxel_arrays) to a scene that prepare_data() has already
        prepared, as one box: the library brings texels, occupancy pyramid and culling box up to date at the box's cost and leaves
        the sky precompute alone (include/vrt_api.h, vrt_update_voxels).  reset: start a fresh accumulation (reset_framebuffer).
        Before the first prepare_data() this IS prepare_data().  No counterpart in the reference."""
        if not getattr(self, "_prepared", False):
            self.prepare_data()
        elif self._voxels_dirty:
            self._push()
            (x0, y0, z0), (x1, y1, z1) = self.dirty_box()
            self._s.update_voxels((x0, y0, z0), (x1, y1, z1), self.voxel_material[x0:x1, y0:y1, z0:z1], self.voxel_color[x0:x1, y0:y1, z0:z1])
            self._voxels_uploaded()
        if reset:
            self.reset_framebuffer()

    # -- asking the scene (include/vrt_api.h, vrt_cast_rays / vrt_fetch_voxels; no counterpart in the reference) -----------------
    def cast_rays(self, origins, dirs, t_max=np.inf, any_hit=False):
        """The reference's next_hit for caller-supplied rays in world units, on the scene as prepare_data() / update_voxels() left it:
        an array of _abi.HIT (t, kind, cell, normal, albedo, mat_id), one record a ray.  origins, dirs: (n, 3) or (3,); t_max and
        any_hit: scalars or one value a ray.  Directions are not normalised: t counts lengths of `dirs`.  `cell` is an array index --
        what voxel_material / voxel_color take, and set_voxel after subtracting voxel_grid_res // 2."""
        if not getattr(self, "_prepared", False):
            raise NativeError("cast_rays asks a prepared scene: call prepare_data() first")
        self._push()
        o = np.asarray(origins, np.float32).reshape(-1, 3)
        rays = np.zeros(len(o), _abi.RAY)
        rays["origin"], rays["dir"], rays["t_max"] = o, np.asarray(dirs, np.float32).reshape(-1, 3), t_max
        rays["flags"] = np.where(np.asarray(any_hit, bool), _abi.RAY_ANY_HIT, 0)
        return self._s.cast_rays(rays)

    # -- moving boxes through the scene (include/vrt_api.h, vrt_sweep_boxes; no counterpart in the reference) ----------------------
    def sweep_boxes(self, lo, hi, move, t_max=1.0, floor=True):
        """Where axis-aligned boxes [lo, hi] (world units) first touch the scene when moved by t * move, 0 <= t < t_max, on the scene as
        prepare_data() / update_voxels() left it: an array of _abi.SWEEP_HIT (t, kind, cell, normal), one record a box.  lo, hi, move:
        (n, 3) or (3,); t_max and floor: scalars or one value a box.  floor=False leaves the floor plane out.  kind is SWEEP_MISS,
        SWEEP_FLOOR, SWEEP_VOXEL or SWEEP_START (the box overlaps something before it moves); the box may move to lo + t * move.
        `cell` is an array index, as cast_rays reports it."""
        if not getattr(self, "_prepared", False):
            raise NativeError("sweep_boxes asks a prepared scene: call prepare_data() first")
        self._push()
        lo = np.asarray(lo, np.float32).reshape(-1, 3)
        boxes = np.zeros(len(lo), _abi.BOX_SWEEP)
        boxes["lo"], boxes["hi"], boxes["move"] = lo, np.asarray(hi, np.float32).reshape(-1, 3), np.asarray(move, np.float32).reshape(-1, 3)
        boxes["t_max"] = t_max
        boxes["flags"] = np.where(np.asarray(floor, bool), 0, _abi.SWEEP_NO_FLOOR)
        return self._s.sweep_boxes(boxes)

    def overlap_boxes(self, lo, hi, floor=True):
        """Whether boxes [lo, hi] overlap a solid voxel or the floor where they stand (a sweep with move = 0; touching is not
        overlapping): (bool[n], int32[n, 3]) -- the first overlapping cell by linear index, -1 for the floor and where nothing overlaps."""
        lo = np.asarray(lo, np.float32).reshape(-1, 3)
        hits = self.sweep_boxes(lo, hi, np.zeros_like(lo), 1.0, floor)
        return hits["kind"] == _abi.SWEEP_START, hits["cell"].copy()

    def box_of_voxels(self, lo_idx, hi_idx):
        """The world-space (lo, hi) of the index box [lo_idx, hi_idx) of array indices -- what update_voxels edits and fetch_voxels
        reads -- exact in float32: an edit box and a sweep box are the same thing."""
        dx = np.float32(2.0 / self.voxel_grid_res)
        lo = np.asarray(lo_idx, np.int64).astype(np.float32) * dx - np.float32(1.0)
        hi = np.asarray(hi_idx, np.int64).astype(np.float32) * dx - np.float32(1.0)
        return lo, hi

    # -- authoring from triangles (include/vrt_api.h, vrt_voxelize_triangles; no counterpart in the reference) ------------------------
    def voxelize_triangles(self, vertices, faces=None, color=(255, 255, 255), mat=1, lo=None, hi=None, reset=True):
        """Voxelise triangles (world units) into the box [lo, hi) of array indices -- by default the whole grid -- of the scene as
        prepare_data() / update_voxels() left it, on the device: every voxel whose closed cube a triangle touches takes that triangle's
        colour and material, later triangles painting over earlier ones; mat = 0 carves.  vertices: (n, 3, 3), or (V, 3) with faces
        (F, 3) of vertex indices; color (r, g, b in 0..255) and mat (the int8 material byte): one value or one per triangle.  A torch
        tensor on the device holding _abi.TRIANGLE records is handed over as it is (faces, color and mat are then not looked at).
        Voxels written with set_voxel and not yet sent go first.  Returns the result record (lo, hi: the tight box of the written
        voxels; voxels; invalid) and brings voxel_material / voxel_color in step over that box (sync_voxels_from_device).  reset:
        start a fresh accumulation."""
        if not getattr(self, "_prepared", False):
            raise NativeError("voxelize_triangles edits a prepared scene: call prepare_data() first")
        if self._voxels_dirty:
            self.update_voxels(reset=False)
        self._push()
        g = self.voxel_grid_res
        lo, hi = ((0, 0, 0) if lo is None else lo), ((g, g, g) if hi is None else hi)
        if hasattr(vertices, "data_ptr"):
            tris = vertices
        else:
            v = np.asarray(vertices, np.float32)
            if faces is not None:
                v = v.reshape(-1, 3)[np.asarray(faces, np.int64).reshape(-1, 3)]
            v = v.reshape(-1, 3, 3)
            tris = np.zeros(len(v), _abi.TRIANGLE)
            tris["v0"], tris["v1"], tris["v2"] = v[:, 0], v[:, 1], v[:, 2]
            c = np.broadcast_to(np.asarray(color, np.int64).reshape(-1, 3), (len(v), 3)).astype(np.uint32) & 0xFF
            m = np.broadcast_to(np.asarray(mat, np.int64).reshape(-1), (len(v),)).astype(np.int8).view(np.uint8).astype(np.uint32)
            tris["voxel"] = c[:, 0] | c[:, 1] << 8 | c[:, 2] << 16 | m << 24
        res = self._s.voxelize_triangles(tris, lo, hi)
        if res["voxels"]:
            self.sync_voxels_from_device(tuple(int(x) for x in res["lo"]), tuple(int(x) for x in res["hi"]))
        if reset:
            self.reset_framebuffer()
        return res

    def fill_triangles(self, vertices, faces=None, color=(255, 255, 255), mat=1, lo=None, hi=None, shell=False, reset=True):
        """Fill the INSIDE of a closed triangle mesh (world units) with one colour (r, g, b in 0..255) and material byte, in the box
        [lo, hi) of array indices -- by default mesh_box(vertices) -- of the scene as prepare_data() / update_voxels() left it, on the
        device (include/vrt_api.h, vrt_fill_triangles): a voxel is inside iff its centre is, by the parity of the triangles below it,
        exactly and whatever their orientation; mat = 0 carves the volume out.  vertices, faces: as for voxelize_triangles; a torch
        tensor on the device holding _abi.TRIANGLE records is handed over as it is (the box is then the whole grid unless given).
        shell=True follows the fill with voxelize_triangles of the same mesh and payload: solid plus conservative skin, every voxel
        the surface touches included (host vertices only).  Returns the result record -- the tight box and the count of the voxels
        written, of fill and skin together with shell=True -- and brings voxel_material / voxel_color in step over that box.  reset:
        start a fresh accumulation."""
        if not getattr(self, "_prepared", False):
            raise NativeError("fill_triangles edits a prepared scene: call prepare_data() first")
        if self._voxels_dirty:
            self.update_voxels(reset=False)
        self._push()
        g = self.voxel_grid_res
        c = [int(x) & 0xFF for x in np.asarray(color, np.int64).reshape(3)]
        voxel = c[0] | c[1] << 8 | c[2] << 16 | int(np.int8(mat).view(np.uint8)) << 24
        if hasattr(vertices, "data_ptr"):
            if shell:
                raise ValueError("shell=True needs the mesh as host vertices: the skin is voxelised with payloads written into the records")
            tris, box = vertices, ((0, 0, 0), (g, g, g))
        else:
            v = np.asarray(vertices, np.float32)
            if faces is not None:
                v = v.reshape(-1, 3)[np.asarray(faces, np.int64).reshape(-1, 3)]
            v = v.reshape(-1, 3, 3)
            tris = np.zeros(len(v), _abi.TRIANGLE)
            tris["v0"], tris["v1"], tris["v2"], tris["voxel"] = v[:, 0], v[:, 1], v[:, 2], voxel
            box = self.mesh_box(v)
        lo, hi = (box[0] if lo is None else lo), (box[1] if hi is None else hi)
        if not shell:
            res = self._s.fill_triangles(tris, lo, hi, voxel)
            if res["voxels"]:
                self.sync_voxels_from_device(tuple(int(x) for x in res["lo"]), tuple(int(x) for x in res["hi"]))
        else:
            res = self._fill_with_shell(tris, lo, hi, voxel)
        if reset:
            self.reset_framebuffer()
        return res

    def _fill_with_shell(self, tris, lo, hi, voxel):
        """Fill plus skin, and the record of their union.  The skin's record counts the cells the surface covers, the fill's the cells
        inside, and many cells are both; to count each once the skin is first written with a payload that no voxel of the box holds, so
        that the host mirror can tell the skin cells the fill leaves over; then the fill, then the skin with the real payload."""
        sl = tuple(slice(int(l), int(h)) for l, h in zip(lo, hi))
        if any(s.stop <= s.start for s in sl) or len(tris) == 0:
            return self._s.fill_triangles(tris, lo, hi, voxel)
        held = self.voxel_color[sl].astype(np.uint32)
        held = np.unique(held[..., 0] | held[..., 1] << 8 | held[..., 2] << 16 | self.voxel_material[sl].view(np.uint8).astype(np.uint32) << 24)
        mark = next(m for m in (voxel & 0xFF000000 | k for k in range(1 << 24)) if m != voxel and m not in held)   # (the box holds at most 2^24 - 1 others only in theory)
        marked = tris.copy()
        marked["voxel"] = mark
        skin = self._s.voxelize_triangles(marked, lo, hi)
        res = self._s.fill_triangles(tris, lo, hi, voxel)
        left = 0
        if skin["voxels"]:
            b = tuple(slice(int(l), int(h)) for l, h in zip(skin["lo"], skin["hi"]))
            self.sync_voxels_from_device(tuple(int(x) for x in skin["lo"]), tuple(int(x) for x in skin["hi"]))
            col = self.voxel_color[b].astype(np.uint32)
            left = int(((col[..., 0] | col[..., 1] << 8 | col[..., 2] << 16 | self.voxel_material[b].view(np.uint8).astype(np.uint32) << 24) == mark).sum())
            self._s.voxelize_triangles(tris, lo, hi)
            if res["voxels"]:
                res["lo"], res["hi"] = np.minimum(res["lo"], skin["lo"]), np.maximum(res["hi"], skin["hi"])
            else:
                res["lo"], res["hi"] = skin["lo"], skin["hi"]
            res["voxels"] += left
        if res["voxels"]:
            self.sync_voxels_from_device(tuple(int(x) for x in res["lo"]), tuple(int(x) for x in res["hi"]))
        return res

    # -- distances (include/vrt_api.h, vrt_distance_field; no counterpart in the reference) --------------------------------------------
    @staticmethod
    def _max_d2(radius):
        """floor(radius^2) of a radius in voxels (may be fractional); None: unbounded"""
        if radius is None:
            return _abi.DIST_MAX_D2
        if not radius >= 0:
            raise ValueError("radius must not be negative")
        return min(int(np.floor(float(radius) * float(radius))), _abi.DIST_MAX_D2)

    def distance_field(self, lo, hi, radius=None, to_empty=False, nearest=False, signed=False):
        """The exact squared distance, in voxels, from every cell of the box [lo, hi) of array indices to the nearest solid voxel of the
        whole grid (to_empty: to the nearest non-solid cell), on the scene as prepare_data() / update_voxels() left it: an int32 array
        of shape hi - lo; beyond `radius` voxels (d2 > floor(radius^2); None: no bound) it holds _abi.DIST_FAR.  nearest=True returns
        (d2, nearest): the linear array index (x * G + y) * G + z of the voxel that attains the distance, the smallest among equals,
        -1 where d2 is DIST_FAR.  signed=True makes both calls and returns +d2 (to the nearest solid) in non-solid cells and -d2 (to the
        nearest non-solid cell) in solid ones, DIST_FAR keeping its sign, with the nearest of whichever applies.  Cells outside the
        grid do not exist: they are neither solid nor empty."""
        if not getattr(self, "_prepared", False):
            raise NativeError("distance_field asks a prepared scene: call prepare_data() first")
        self._push()
        md = self._max_d2(radius)
        if not signed:
            return self._s.distance_field(lo, hi, md, to_empty=to_empty, nearest=nearest)
        out, inn = (self._s.distance_field(lo, hi, md, to_empty=e, nearest=True) for e in (False, True))
        outside = out[0] > 0                                   # a solid cell is its own nearest solid
        d2 = np.where(outside, out[0], -inn[0]).astype(np.int32)
        return (d2, np.where(outside, out[1], inn[1]).astype(np.int32)) if nearest else d2

    def _box_on_device(self, lo, hi, md, to_empty, nearest):
        """(d2, nearest or None, mat, rgb) of the box as torch tensors on the device, computed and waited for"""
        import torch
        shape = tuple(int(h) - int(l) for l, h in zip(lo, hi))
        d2 = torch.empty(shape, dtype=torch.int32, device="cuda")
        near = torch.empty(shape, dtype=torch.int32, device="cuda") if nearest else None
        mat, rgb = torch.empty(shape, dtype=torch.int8, device="cuda"), torch.empty(shape + (3,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                               # (allocations are torch's; the library writes on the session's stream)
        self._s.distance_field(lo, hi, md, to_empty=to_empty, nearest=nearest, out=(d2, near) if nearest else d2)
        self._s.fetch_voxels(lo, hi, mat.data_ptr(), rgb.data_ptr(), on_device=True)
        self._s.sync()
        return d2, near, mat, rgb

    def _edit_from_device(self, lo, hi, mat, rgb, reset):
        import torch
        mat, rgb = mat.contiguous(), rgb.contiguous()
        torch.cuda.synchronize()                               # (written on torch's stream, read on the session's)
        self._s.update_voxels(lo, hi, mat.data_ptr(), rgb.data_ptr(), on_device=True)   # (waits for the edit: the tensors may go)
        self.sync_voxels_from_device(tuple(int(v) for v in lo), tuple(int(v) for v in hi))
        if reset:
            self.reset_framebuffer()

    def grow_voxels(self, lo, hi, radius, color=None, mat=None, reset=True):
        """Grow the solids by `radius` voxels inside the box [lo, hi) of array indices, on the device: every non-solid cell of the box
        whose squared distance to the nearest solid voxel of the grid is <= floor(radius^2) becomes solid (distance_field and
        fetch_voxels into device tensors, torch.where, update_voxels from device memory).  color (r, g, b in 0..255) and mat: the new
        voxels' payload; with None the colour / material of the cell's nearest solid voxel -- the smallest linear index among equally
        near ones -- is inherited.  Solids outside the box count as sources; only cells of the box are written.  Cells outside the grid
        do not exist.  Returns the number of cells that became solid and brings voxel_material / voxel_color in step over the box.
        reset: start a fresh accumulation."""
        import torch
        if not getattr(self, "_prepared", False):
            raise NativeError("grow_voxels edits a prepared scene: call prepare_data() first")
        if self._voxels_dirty:
            self.update_voxels(reset=False)
        self._push()
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        if any(h <= l for l, h in zip(lo, hi)):
            return 0
        md = self._max_d2(radius)
        inherit = color is None or mat is None
        d2, near, bm, bc = self._box_on_device(lo, hi, md, False, inherit)
        grow = (bm <= 0) & (d2 <= md)
        new_m = torch.full_like(bm, int(np.int8(mat))) if mat is not None else None
        new_c = torch.tensor([int(x) & 0xFF for x in np.asarray(color, np.int64).reshape(3)], dtype=torch.uint8, device="cuda").expand(bc.shape) if color is not None else None
        if inherit:                                            # the nearest solid lies within floor(radius) of the box: fetch that much
            g, r = self.voxel_grid_res, int(np.floor(np.sqrt(md)))
            while (r + 1) * (r + 1) <= md:
                r += 1
            glo, ghi = [max(l - r, 0) for l in lo], [min(h + r, g) for h in hi]
            gs = [h - l for l, h in zip(glo, ghi)]
            gm, gc = torch.empty(gs, dtype=torch.int8, device="cuda"), torch.empty(gs + [3], dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            self._s.fetch_voxels(glo, ghi, gm.data_ptr(), gc.data_ptr(), on_device=True)
            self._s.sync()
            n = torch.where(grow, near, torch.zeros_like(near)).long()
            x, y, z = n // (g * g), (n // g) % g, n % g
            at = torch.where(grow, ((x - glo[0]) * gs[1] + (y - glo[1])) * gs[2] + (z - glo[2]), torch.zeros_like(n)).reshape(-1)
            if new_m is None:
                new_m = gm.reshape(-1)[at].reshape(bm.shape)
            if new_c is None:
                new_c = gc.reshape(-1, 3)[at].reshape(bc.shape)
        count = int(grow.sum().item())
        self._edit_from_device(lo, hi, torch.where(grow, new_m, bm), torch.where(grow[..., None], new_c, bc), reset)
        return count

    def shrink_voxels(self, lo, hi, radius, reset=True):
        """Shrink the solids by `radius` voxels inside the box [lo, hi) of array indices, on the device: every solid cell of the box whose
        squared distance to the nearest non-solid cell of the grid is <= floor(radius^2) becomes empty (material 0, colour 0).  Cells
        outside the grid do not exist, so they are not empty either: a solid pressed against the grid's wall is not eroded from that
        side.  Non-solid cells outside the box count as sources; only cells of the box are written.  Returns the number of cells that
        became empty and brings voxel_material / voxel_color in step over the box.  reset: start a fresh accumulation."""
        import torch
        if not getattr(self, "_prepared", False):
            raise NativeError("shrink_voxels edits a prepared scene: call prepare_data() first")
        if self._voxels_dirty:
            self.update_voxels(reset=False)
        self._push()
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        if any(h <= l for l, h in zip(lo, hi)):
            return 0
        md = self._max_d2(radius)
        d2, _, bm, bc = self._box_on_device(lo, hi, md, True, False)
        gone = (bm > 0) & (d2 <= md)
        count = int(gone.sum().item())
        self._edit_from_device(lo, hi, torch.where(gone, torch.zeros_like(bm), bm), torch.where(gone[..., None], torch.zeros_like(bc), bc), reset)
        return count

    # -- what hangs together (include/vrt_api.h, vrt_label_components; no counterpart in the reference) ----------------------------------
    def _label_box(self, what, lo, hi):
        if not getattr(self, "_prepared", False):
            raise NativeError(f"{what} asks a prepared scene: call prepare_data() first")
        if self._voxels_dirty:
            self.update_voxels(reset=False)
        self._push()
        g = self.voxel_grid_res
        return [int(v) for v in ((0, 0, 0) if lo is None else lo)], [int(v) for v in ((g, g, g) if hi is None else hi)]

    def label_components(self, lo=None, hi=None, connectivity=6, empty=False):
        """The connected components of the solid voxels of the box [lo, hi) of array indices -- by default the whole grid -- on the
        scene as prepare_data() / update_voxels() left it (voxels written with set_voxel and not yet sent go first): (labels, result).
        labels: an int32 array of shape hi - lo, every solid cell holding the smallest linear array index (x * G + y) * G + z of its
        component, every other cell -1; result: the dict of `cells` (solid cells) and `components`.  connectivity: 6 (faces), 18 (and
        edges) or 26 (and corners).  empty=True labels the non-solid cells instead.  Cells outside the box do not exist: a piece that
        continues outside it is cut at its faces."""
        lo, hi = self._label_box("label_components", lo, hi)
        return self._s.label_components(lo, hi, connectivity, empty)

    def _labels_on_device(self, lo, hi, connectivity, empty):
        """the labels of the box as a torch tensor on the device, computed and waited for"""
        import torch
        labels = torch.empty(tuple(max(h - l, 0) for l, h in zip(lo, hi)), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                               # (allocations are torch's; the library writes on the session's stream)
        self._s.label_components(lo, hi, connectivity, empty, out=labels)
        self._s.sync()
        return labels

    def components(self, lo=None, hi=None, connectivity=6, empty=False):
        """The table of the components label_components finds, computed on the device (torch.unique and scatter_reduce over the labels)
        and sorted by root: a dict of device tensors -- root int32[n], the component's smallest linear array index; size int64[n], its
        cells; lo, hi int32[n, 3], its tight box [lo, hi) of array indices."""
        import torch
        lo, hi = self._label_box("components", lo, hi)
        labels = self._labels_on_device(lo, hi, connectivity, empty)
        at = torch.nonzero(labels >= 0)                                                         # box-local coordinates, int64[m, 3]
        root, inverse, size = torch.unique(labels[labels >= 0], return_inverse=True, return_counts=True)
        cells = (at + torch.tensor(lo, device="cuda")).to(torch.int32)
        where = inverse[:, None].expand(-1, 3)
        big = torch.iinfo(torch.int32).max
        c_lo = torch.full((len(root), 3), big, dtype=torch.int32, device="cuda").scatter_reduce(0, where, cells, "amin")
        c_hi = torch.full((len(root), 3), -1, dtype=torch.int32, device="cuda").scatter_reduce(0, where, cells, "amax") + 1
        return dict(root=root, size=size, lo=c_lo, hi=c_hi)

    def floating_voxels(self, lo, hi, connectivity=6):
        """What would fall: a boolean device tensor of shape hi - lo marking the solid cells of the box [lo, hi) whose component -- cut
        at the box's faces -- has no cell in the box's lowest layer y == lo[1] (the world's up is y).  Put the box's lowest layer on
        what carries the scene (the ground, a slab): what is joined to it stands, the rest floats."""
        import torch
        lo, hi = self._label_box("floating_voxels", lo, hi)
        labels = self._labels_on_device(lo, hi, connectivity, False)
        if labels.numel() == 0:
            return labels >= 0
        ground = labels[:, 0, :]
        return (labels >= 0) & ~torch.isin(labels, torch.unique(ground[ground >= 0]))

    def remove_floating(self, lo, hi, connectivity=6, reset=True):
        """Carve floating_voxels(lo, hi, connectivity) out of the grid (material 0, colour 0), on the device.  Returns the number of
        cells that became empty and brings voxel_material / voxel_color in step over the box.  reset: start a fresh accumulation."""
        import torch
        gone = self.floating_voxels(lo, hi, connectivity)
        count = int(gone.sum().item())
        if count == 0:
            return 0
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        bm, bc = torch.empty(gone.shape, dtype=torch.int8, device="cuda"), torch.empty(tuple(gone.shape) + (3,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self._s.fetch_voxels(lo, hi, bm.data_ptr(), bc.data_ptr(), on_device=True)
        self._s.sync()
        self._edit_from_device(lo, hi, torch.where(gone, torch.zeros_like(bm), bm), torch.where(gone[..., None], torch.zeros_like(bc), bc), reset)
        return count

    # -- moving what is there (include/vrt_api.h, vrt_move_voxels; no counterpart in the reference) ---------------------------------------
    @staticmethod
    def rotation_matrix(axis, degrees):
        """The 3x3 rotation by `degrees` about `axis` ("x", "y", "z" or a 3-vector), float64; a multiple of 90 degrees about a
        coordinate axis comes out in exact integers."""
        axis = {"x": (1.0, 0.0, 0.0), "y": (0.0, 1.0, 0.0), "z": (0.0, 0.0, 1.0)}.get(axis, axis) if isinstance(axis, str) else axis
        k = np.asarray(axis, np.float64)
        k = k / np.linalg.norm(k)
        q = float(degrees) / 90.0
        c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(q) % 4] if q == int(q) else (np.cos(np.radians(degrees)), np.sin(np.radians(degrees)))
        K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        return np.eye(3) * c + s * K + (1.0 - c) * np.outer(k, k)

    @staticmethod
    def move_transform(rotation=None, pivot=None, shift=(0, 0, 0)):
        """(m, t) of vrt_move_voxels for the FORWARD map p' = R (p - pivot) + pivot + shift in array-index space (a cell's centre is
        its index + 0.5; pivot and shift may be fractional; R any invertible 3x3, by default the identity): the map is inverted in
        float64 and rounded here -- m = rint(R^-1 * 2^16), t = rint((pivot - R^-1 (pivot + shift)) * 2^17) -- and the library sees the
        integers only."""
        R = np.eye(3) if rotation is None else np.asarray(rotation, np.float64).reshape(3, 3)
        pivot = np.zeros(3) if pivot is None else np.asarray(pivot, np.float64).reshape(3)
        shift = np.asarray(shift, np.float64).reshape(3)
        inv = np.linalg.inv(R)
        m = np.rint(inv * 65536.0).astype(np.int64)
        t = np.rint((pivot - inv @ (pivot + shift)) * 131072.0).astype(np.int64)
        return m, t

    def moved_box(self, src_lo, src_hi, rotation=None, pivot=None, shift=(0, 0, 0)):
        """Where the source box [src_lo, src_hi) goes under the forward map of move_transform: the bounds of its eight mapped corners,
        grown by one cell and clipped to the grid -- (lo, hi) of array indices, the default destination box of move_voxels."""
        R = np.eye(3) if rotation is None else np.asarray(rotation, np.float64).reshape(3, 3)
        pivot = np.zeros(3) if pivot is None else np.asarray(pivot, np.float64).reshape(3)
        shift = np.asarray(shift, np.float64).reshape(3)
        corners = np.array([[(src_lo, src_hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)], np.float64)
        image = (corners - pivot) @ R.T + pivot + shift
        g = self.voxel_grid_res
        lo = np.clip(np.floor(image.min(0)).astype(np.int64) - 1, 0, g)
        hi = np.clip(np.ceil(image.max(0)).astype(np.int64) + 1, 0, g)
        return tuple(int(v) for v in lo), tuple(int(v) for v in np.maximum(hi, lo))

    def move_voxels(self, src_lo, src_hi, rotation=None, pivot=None, shift=(0, 0, 0), select=None, select_value=0, copy=False, keep_solid=False,
                    if_free=False, dry_run=False, dst_lo=None, dst_hi=None, reset=True):
        """Move the solid voxels of the box [src_lo, src_hi) of array indices by p' = rotation (p - pivot) + pivot + shift, on the device
        (include/vrt_api.h, vrt_move_voxels): every cell of the destination box [dst_lo, dst_hi) -- by default moved_box(...) -- whose
        centre maps back into a solid, selected cell of the source box takes that cell's material and colour, and the source's cells
        are emptied (copy=True: they stay).  select: an int32 array or device tensor of the source box's shape, e.g. the labels of
        label_components over the same box; only cells equal to select_value take part.  keep_solid: solid cells in the way keep
        their voxel; if_free: nothing at all happens if a solid cell is in the way; dry_run: only the counts.  Nearest-neighbour
        resampling: turns by multiples of 90 degrees about a pivot that maps cell centres to cell centres are exact, any other map
        may lose or double voxels (compare written and erased).  Returns the dict of lo, hi (the tight box written), written, blocked
        (solid cells that were in the way) and erased, and brings voxel_material / voxel_color in step over both boxes.  reset: start a
        fresh accumulation if the grid changed."""
        lo, hi = self._label_box("move_voxels", src_lo, src_hi)
        m, t = self.move_transform(rotation, pivot, shift)
        box = self.moved_box(lo, hi, rotation, pivot, shift)
        dst_lo = [int(v) for v in (box[0] if dst_lo is None else dst_lo)]
        dst_hi = [int(v) for v in (box[1] if dst_hi is None else dst_hi)]
        flags = ((0 if copy else _abi.MOVE_ERASE_SOURCE) | (_abi.MOVE_KEEP_SOLID if keep_solid else 0) | (_abi.MOVE_IF_FREE if if_free else 0)
                 | (_abi.MOVE_DRY_RUN if dry_run else 0))
        if select is not None and not hasattr(select, "data_ptr"):
            select = np.ascontiguousarray(select, np.int32)
        res = self._s.move_voxels(lo, hi, dst_lo, dst_hi, m, t, flags, select, select_value)
        if not dry_run and (res["written"] or res["erased"]):
            if res["erased"]:
                self.sync_voxels_from_device(lo, hi)
            if res["written"]:
                self.sync_voxels_from_device(res["lo"], res["hi"])
            if reset:
                self.reset_framebuffer()
        return res

    def copy_voxels(self, src_lo, src_hi, **kwargs):
        """move_voxels(copy=True): the source keeps its voxels."""
        return self.move_voxels(src_lo, src_hi, copy=True, **kwargs)

    def sealed_cavities(self, lo, hi):
        """The cells a flood from outside cannot reach: a boolean device tensor of shape hi - lo marking the non-solid cells of the box
        [lo, hi) whose 6-connected component of non-solid cells touches no face of the box."""
        import torch
        lo, hi = self._label_box("sealed_cavities", lo, hi)
        labels = self._labels_on_device(lo, hi, 6, True)
        if labels.numel() == 0:
            return labels >= 0
        faces = torch.cat([f.reshape(-1) for f in (labels[0], labels[-1], labels[:, 0], labels[:, -1], labels[:, :, 0], labels[:, :, -1])])
        return (labels >= 0) & ~torch.isin(labels, torch.unique(faces[faces >= 0]))

    def mesh_box(self, vertices):
        """The box [lo, hi) of array indices that encloses every voxel a mesh with these vertices (world units, any shape (..., 3)) can
        cover, clamped to the grid: what voxelize_triangles takes as lo, hi.  A vertex on a grid plane counts the cells on both sides.
        Vertices with a non-finite component are left out (the library skips their triangles); with none left the box is empty."""
        g = self.voxel_grid_res
        v = np.asarray(vertices, np.float32).reshape(-1, 3)
        v = np.clip(v[np.isfinite(v).all(axis=1)], -_abi.TRI_MAX_COORD, _abi.TRI_MAX_COORD)
        if len(v) == 0:
            return (0, 0, 0), (0, 0, 0)
        s = np.rint((v + np.float32(1.0)) * np.float32(g // 2) * np.float32(64.0)).astype(np.int64)   # the library's snap: 64ths of a voxel
        lo = np.clip((s.min(axis=0) - 1) >> 6, 0, g)
        hi = np.clip((s.max(axis=0) >> 6) + 1, 0, g)
        return tuple(int(x) for x in lo), tuple(int(x) for x in np.maximum(hi, lo))

    def pick_ray(self, u, v):
        """(origin, direction) of the ray through the centre of pixel (u, v), v = 0 at the bottom: get_cast_dir (pathtracer.py:293-312)
        without the TAA jitter, statement by statement in float32, from the matrices and the position the renderer was last given."""
        self._push()
        f = np.float32
        view_inv, proj_inv = cam_mod.inverse_f32(self._view), cam_mod.inverse_f32(self._proj)
        W, H = self.image_res
        scale = f(self._render_scale)
        tx = (f(u) + f(0.5)) * f(1.0 / W) / scale
        ty = (f(v) + f(0.5)) * f(1.0 / H) / scale
        pos = (tx * f(2.0) - f(1.0), ty * f(2.0) - f(1.0), f(1.0) * f(2.0) - f(1.0), f(1.0))            # screen_to_view, depth 1

        def mul(M, p):
            return [M[i, 0] * p[0] + M[i, 1] * p[1] + M[i, 2] * p[2] + M[i, 3] * p[3] for i in range(4)]
        q = mul(proj_inv, pos)
        d = [q[0] / q[3], q[1] / q[3], q[2] / q[3]]
        inv = f(1.0) / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])                                 # Vector.normalized()
        d = [inv * d[0], inv * d[1], inv * d[2]]
        w = mul(view_inv, (d[0], d[1], d[2], f(0.0)))                                                   # view_to_world, a direction
        return np.array(self._pos, np.float32), np.array(w[:3], np.float32)

    def pick(self, u, v, t_max=np.inf):
        """The hit record under pixel (u, v): cast_rays(*pick_ray(u, v))[0]."""
        o, d = self.pick_ray(u, v)
        return self.cast_rays(o, d, t_max)[0]

    # -- how much light arrives along a ray (include/vrt_api.h, vrt_trace_radiance; no counterpart in the reference) ---------------
    def trace_radiance(self, origins, dirs, samples=1, first_frame=0, streams=None, normalize=True):
        """Path-traced radiance along caller-supplied rays in world units, on the scene as prepare_data() / update_voxels() left it: a
        structured array (`rgb`: the mean of `samples` samples; `t`: the distance of the first hit, inf into the sky), one record a
        ray.  origins, dirs: (n, 3) or (3,), numpy arrays or torch tensors on the device (those go through the device path: the records
        are put together on the device and only the result comes back).  The estimator takes `dirs` for unit vectors: normalize=True
        normalises them in float64 before the cast to float32, normalize=False passes them on bit for bit.  Sample s of ray k draws
        from random stream (seed, first_frame + s, streams[k], 0); streams defaults to arange(n), so two calls with the same arguments
        return the same bits and first_frame = samples continues where a call left off."""
        if not getattr(self, "_prepared", False):
            raise NativeError("trace_radiance asks a prepared scene: call prepare_data() first")
        self._push()
        if hasattr(origins, "data_ptr") or hasattr(dirs, "data_ptr"):
            import torch
            dev = origins.device if hasattr(origins, "data_ptr") else dirs.device
            o = torch.as_tensor(origins, device=dev).to(torch.float32).reshape(-1, 3)
            d = torch.as_tensor(dirs, device=dev).reshape(-1, 3)
            if normalize:
                d = d.to(torch.float64)
                d = d / torch.linalg.norm(d, dim=1, keepdim=True)
            n = max(o.shape[0], d.shape[0])
            rec = torch.zeros((n, 8), dtype=torch.float32, device=dev)
            rec[:, 0:3], rec[:, 4:7] = o, d.to(torch.float32)
            st = torch.arange(n, device=dev, dtype=torch.int64) if streams is None else torch.as_tensor(streams, device=dev).to(torch.int64).reshape(-1)
            rec.view(torch.int32)[:, 3] = (((st & 0xFFFFFFFF) + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)   # the stream's 32 bits
            out = torch.empty((n, 4), dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)               # the tensors are written on torch's stream, read on the session's
            self._s.trace_radiance(rec, samples, first_frame, out)
            self._s.sync()
            return out.cpu().numpy().view(_abi.RADIANCE).reshape(-1)
        o = np.asarray(origins, np.float32).reshape(-1, 3)
        d = np.asarray(dirs).reshape(-1, 3)
        if normalize:
            d = d.astype(np.float64)
            d = d / np.linalg.norm(d, axis=1, keepdims=True)
        rays = np.zeros(max(len(o), len(d)), _abi.PATH_RAY)
        rays["origin"], rays["dir"] = o, d.astype(np.float32)
        rays["stream"] = np.arange(len(rays), dtype=np.uint32) if streams is None else np.asarray(streams).astype(np.uint32)
        return self._s.trace_radiance(rays, samples, first_frame)

    # -- how much light falls on a surface point (include/vrt_api.h, vrt_gather_irradiance; no counterpart in the reference) ---------
    def gather_irradiance(self, points, normals, samples=64, first_frame=0, streams=None):
        """Irradiance at caller-supplied surface points in world units, on the scene as prepare_data() / update_voxels() left it: a
        structured array of _abi.IRRADIANCE, one record a point -- sky_rgb (the hemisphere's light, sky and bounced), sky (the open share
        of the cosine-weighted hemisphere), sun_rgb (the sun's direct light), sun (the visible share of its disc), each the mean of
        `samples` samples; the total is sky_rgb + sun_rgb.  points, normals: (n, 3) or (3,), numpy arrays or torch tensors on the device
        (those go through the device path).  Normals are taken for unit vectors and passed on bit for bit.  Sample s of point k draws
        from random streams (seed, first_frame + s, streams[k], 4) and (.., 0); streams defaults to arange(n)."""
        if not getattr(self, "_prepared", False):
            raise NativeError("gather_irradiance asks a prepared scene: call prepare_data() first")
        self._push()
        if hasattr(points, "data_ptr") or hasattr(normals, "data_ptr"):
            import torch
            dev = points.device if hasattr(points, "data_ptr") else normals.device
            o = torch.as_tensor(points, device=dev).to(torch.float32).reshape(-1, 3)
            d = torch.as_tensor(normals, device=dev).to(torch.float32).reshape(-1, 3)
            n = max(o.shape[0], d.shape[0])
            rec = torch.zeros((n, 8), dtype=torch.float32, device=dev)
            rec[:, 0:3], rec[:, 4:7] = o, d
            st = torch.arange(n, device=dev, dtype=torch.int64) if streams is None else torch.as_tensor(streams, device=dev).to(torch.int64).reshape(-1)
            rec.view(torch.int32)[:, 3] = (((st & 0xFFFFFFFF) + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)   # the stream's 32 bits
            out = torch.empty((n, 8), dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)               # the tensors are written on torch's stream, read on the session's
            self._s.gather_irradiance(rec, samples, first_frame, out)
            self._s.sync()
            return out.cpu().numpy().view(_abi.IRRADIANCE).reshape(-1)
        o = np.asarray(points, np.float32).reshape(-1, 3)
        d = np.asarray(normals, np.float32).reshape(-1, 3)
        sensors = np.zeros(max(len(o), len(d)), _abi.SENSOR)
        sensors["pos"], sensors["normal"] = o, d
        sensors["stream"] = np.arange(len(sensors), dtype=np.uint32) if streams is None else np.asarray(streams).astype(np.uint32)
        return self._s.gather_irradiance(sensors, samples, first_frame)

    def bake_faces(self, lo=None, hi=None, samples=64):
        """surface_faces(lo, hi) followed by gather_irradiance at the faces' centres: (cell, face, irradiance records), stream k for
        face k of the list."""
        cell, face, centre, normal = self.surface_faces(lo, hi)
        return cell, face, self.gather_irradiance(centre, normal, samples=samples)

    # -- the light at points in empty space (include/vrt_api.h, vrt_gather_probes; no counterpart in the reference) -------------------
    def gather_probes(self, points, samples=64, first_frame=0, streams=None):
        """Spherical-harmonic light probes at caller-supplied points in world units, on the scene as prepare_data() / update_voxels()
        left it: a structured array of _abi.SH_PROBE, one record a point -- sh (nine coefficients per colour channel of the arriving
        radiance, sun excluded; polar axis z, the world's up is y), sky (the open share of the sphere), sun_rgb (the sun's irradiance on
        a surface that faces it), sun (the visible share of its disc), each the mean of `samples` samples.  sh_irradiance / sh_radiance
        read the records.  points: (n, 3) or (3,), a numpy array or a torch tensor on the device (that goes through the device path).
        Sample s of point k draws from random streams (seed, first_frame + s, streams[k], 5) and (.., 0); streams defaults to arange(n)."""
        if not getattr(self, "_prepared", False):
            raise NativeError("gather_probes asks a prepared scene: call prepare_data() first")
        self._push()
        if hasattr(points, "data_ptr"):
            import torch
            dev = points.device
            o = points.to(torch.float32).reshape(-1, 3)
            n = o.shape[0]
            rec = torch.zeros((n, 4), dtype=torch.float32, device=dev)
            rec[:, 0:3] = o
            st = torch.arange(n, device=dev, dtype=torch.int64) if streams is None else torch.as_tensor(streams, device=dev).to(torch.int64).reshape(-1)
            rec.view(torch.int32)[:, 3] = (((st & 0xFFFFFFFF) + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)   # the stream's 32 bits
            out = torch.empty((n, 32), dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)               # the tensors are written on torch's stream, read on the session's
            self._s.gather_probes(rec, samples, first_frame, out)
            self._s.sync()
            return out.cpu().numpy().view(_abi.SH_PROBE).reshape(-1)
        o = np.asarray(points, np.float32).reshape(-1, 3)
        probes = np.zeros(len(o), _abi.PROBE)
        probes["pos"] = o
        probes["stream"] = np.arange(len(probes), dtype=np.uint32) if streams is None else np.asarray(streams).astype(np.uint32)
        return self._s.gather_probes(probes, samples, first_frame)

    @staticmethod
    def panorama_dirs(width, height):
        """The unit directions of an equirectangular image, float64[height][width][3]: pixel (row i, column j) looks along longitude
        phi = 2 pi (j + 0.5) / width - pi (phi = 0 is -z, the default camera's forward; +x is to the right) and latitude
        theta = pi / 2 - pi (i + 0.5) / height (row 0 at the top, looking up): (cos theta sin phi, sin theta, -cos theta cos phi)."""
        phi = 2.0 * np.pi * (np.arange(width) + 0.5) / width - np.pi
        theta = 0.5 * np.pi - np.pi * (np.arange(height) + 0.5) / height
        ct, st = np.cos(theta)[:, None], np.sin(theta)[:, None]
        return np.stack([ct * np.sin(phi)[None, :], np.broadcast_to(st, (height, width)), -ct * np.cos(phi)[None, :]], axis=-1)

    def render_panorama(self, origin, width, height, samples):
        """An equirectangular 360-degree image of the radiance arriving at `origin`, float32[height][width][3] (linear HDR): pixel
        (i, j) is trace_radiance(origin, panorama_dirs(width, height)[i, j], samples) with stream i * width + j."""
        dirs = self.panorama_dirs(width, height).reshape(-1, 3)
        got = self.trace_radiance(np.broadcast_to(np.asarray(origin, np.float32), dirs.shape), dirs, samples=samples)
        return got["rgb"].reshape(height, width, 3).copy()

    def tone_map(self, hdr):
        """The presentation curve of fetch_image (pathtracer.py:634-662: exposure, uchimura of math_utils.py:163-186, gamma 2.2) without its
        vignette, in numpy, for HDR images that do not come from the camera (render_panorama): float rgba [H, W, 4] for save_image."""
        x = np.asarray(hdr, np.float32) * np.float32(self.exposure)
        x = np.clip(np.nan_to_num(x, nan=0.0, posinf=1e6, neginf=0.0), 0.0, 1e6).astype(np.float64)   # (black for NaN and negative light, white for unbounded)
        P, a, m, l, c, b = 1.0, 1.0, 0.22, 0.4, 1.33, 0.0
        l0 = ((P - m) * l) / a
        S0, S1 = m + l0, m + a * l0
        CP = -((a * P) / (P - S1)) / P
        w0 = 1.0 - (lambda t: t * t * (3.0 - 2.0 * t))(np.clip(x / m, 0.0, 1.0))
        w2 = np.where(x < m + l0, 0.0, 1.0)
        w1 = 1.0 - w0 - w2
        with np.errstate(invalid="ignore", over="ignore"):
            T = m * np.power(x / m, c) + b
            S = P - (P - S1) * np.exp(CP * (x - S0))
        L = m + a * (x - m)
        rgb = np.clip(np.power(np.clip(T * w0 + L * w1 + S * w2, 0.0, None), 1.0 / 2.2), 0.0, 1.0)
        return np.concatenate([rgb, np.ones(rgb.shape[:-1] + (1,))], axis=-1).astype(np.float32)

    def sync_voxels_from_device(self, lo=None, hi=None):
        """Refresh voxel_material / voxel_color (what get_voxel reads) in the box [lo, hi) of array indices -- by default the whole
        grid -- from the device, after edits the host never saw (NativeSession.update_voxels with device memory).  The voxels
        are not marked dirty: they are what the device holds.  Voxels written with set_voxel since the last upload and not yet sent
        are overwritten inside the box."""
        if not getattr(self, "_prepared", False):
            raise NativeError("sync_voxels_from_device reads a prepared scene: call prepare_data() first")
        g = self.voxel_grid_res
        (x0, y0, z0), (x1, y1, z1) = (lo if lo is not None else (0, 0, 0)), (hi if hi is not None else (g, g, g))
        mat, rgb = self._s.fetch_voxels((x0, y0, z0), (x1, y1, z1))
        self.voxel_material[x0:x1, y0:y1, z0:z1] = mat
        self.voxel_color[x0:x1, y0:y1, z0:z1] = rgb

    def accumulate_clouds(self, max_samples):
        self._push()
        self._s.sky_accumulate_clouds(max_samples)

    def compute_atmosphere(self, slice_idx, max_slices):
        self._push()
        self._s.sky_compute_slice(slice_idx, max_slices)

    def reset_framebuffer(self):
        self.current_spp = 0
        self._s.reset()

    def accumulate(self, n=1):
        self._push()
        self._s.accumulate(n)
        self.current_spp += n
        self.current_frame += n

    def fetch_image(self):
        """LDR rgba float32 [H, W, 4] (row 0 = bottom, like the reference's (u, v) image)."""
        self._push()
        return self._s.fetch_ldr()

    def fetch_hdr(self):
        return self._s.fetch_hdr()

    def fetch_denoised(self, iterations=5, plane_tolerance=0.25, sigma_l=0.5, full_at=64.0, ldr=False):
        """The accumulated frame through the g-buffer-guided spatial filter (include/vrt_api.h, vrt_denoise), for frames with few samples
        behind them -- after an edit and a reset, behind a moving camera: linear HDR float32 [H, W, 3] (row 0 = bottom), the counterpart
        of fetch_hdr().  `iterations` a-trous passes (1 .. 6, strides 1, 2, 4, ..); taps further than `plane_tolerance` voxels from the
        centre pixel's plane are left out; `sigma_l` is the luminance stopping's relative width (0: off); a pixel with `full_at` samples
        or more gets its unfiltered value (0: always the filtered one).  The defaults are a matter of taste: nobody has validated them
        on images.  With ldr=True the result is tone_map(hdr) -- the numpy presentation curve WITHOUT fetch_image's vignette -- as
        float rgba [H, W, 4] for save_image.  Nothing is written back: the accumulation goes on as if the call had not been made."""
        hdr = self._s.denoise(_abi.VrtDenoiseParams(iterations, plane_tolerance, sigma_l, full_at))
        return self.tone_map(hdr) if ldr else hdr

    def set_reference_indexing(self, on=True):
        """Occupancy queries outside the grid read the bit the reference's index arithmetic addresses (raytracer.py:17-38)
        instead of "empty" (the default).  Also `VRT_REFERENCE_INDEXING=1` in the environment."""
        self._s.set_reference_indexing(on)

    # The reference shows every frame (scene.py:255-262: accumulate, fetch_image, canvas.set_image).  A blocking fetch_image
    # waits for every launch queued so far; these two queue the tonemap and the copy of an 8-bit image behind the frame and
    # return, so the caller can queue the next frame and pick the image up a frame later (two slots alternate).
    def present_async(self, slot=0):
        self._push()
        if not hasattr(self, "_present"):
            self._present = [self._s.host_alloc((self.image_res[1], self.image_res[0], 4), np.uint8) for _ in range(2)]
        self._s.fetch_ldr8_async(self._present[slot & 1], slot & 1)

    def present_wait(self, slot=0):
        """rgba8 [H, W, 4] (row 0 = bottom) of the frame present_async(slot) was called on.  A copy: the page-locked buffer
        behind it is reused two frames later and is freed when the session closes."""
        self._s.fetch_wait(slot & 1)
        return self._present[slot & 1].copy()

    def stats(self):
        return self._s.stats()

    @property
    def session(self):
        return self._s
