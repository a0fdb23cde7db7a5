"""Triangle meshes onto the terrace of moving_box.py: a torus and an icosphere are built in numpy (no asset files), voxelised into
the prepared scene on the device (Renderer.voxelize_triangles -> vrt_voxelize_triangles), and a second, smaller sphere is carved out of
the torus with mat = 0.  Each call edits the box that encloses its mesh (Renderer.mesh_box) and brings the host's voxel arrays in step.
Headless; new code, not one of the reference's scripts.  Run from the repo root:

    VRT_RES=640x360 VRT_FRAMES=16 VRT_SPP=4 VRT_SKY_RES=512 python examples/voxelize_mesh.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scene import Scene, save_image  # noqa: E402


def torus(centre, major, minor, nu=48, nv=24):
    """(vertices (V, 3), faces (F, 3)) of a torus around the y axis, world units"""
    u, v = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    ring = major + minor * np.cos(v)
    pts = np.stack([ring * np.cos(u), minor * np.sin(v), ring * np.sin(u)], axis=-1).reshape(-1, 3) + np.asarray(centre)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    faces = [t for i in range(nu) for j in range(nv) for t in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))]
    return pts, np.array(faces)


def icosphere(centre, radius, subdivisions):
    """(vertices, faces) of an icosahedron whose triangles are split in four `subdivisions` times, pushed out to the sphere"""
    g = (1 + 5 ** 0.5) / 2
    v = [np.array(p, float) / np.linalg.norm(p) for p in ((-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
                                                           (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1))]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius + np.asarray(centre), np.array(f)


def main():
    spp = int(os.environ.get("VRT_SPP", 4))
    frames = int(os.environ.get("VRT_FRAMES", 16))
    scene = Scene(voxel_edges=0.0, exposure=2.0)
    scene.set_floor(-0.85, (1.0, 1.0, 1.0))
    scene.set_directional_light((1, 1, -1), 0.025, (1.3, 1.23, 1.22))
    scene.set_use_physical_sky(True)
    scene.set_use_clouds(True)
    r = scene.renderer

    for x in range(-48, 49):                 # the terrace with its low wall
        for z in range(-48, 49):
            edge = max(abs(x), abs(z)) == 48
            for y in range(-40, -36 if edge else -38):
                scene.set_voxel((x, y, z), 11, (0.55, 0.5, 0.45) if (x // 8 + z // 8) % 2 else (0.7, 0.65, 0.6))
    r.prepare_data()
    for _ in range(8):
        r.accumulate_clouds(8)
    for s in range(8):
        r.compute_atmosphere(s, 8)

    dx = 2.0 / r.voxel_grid_res
    results = {}
    tv, tf = torus((0.0, -26.5 * dx, 0.0), 22.3 * dx, 7.6 * dx)                    # lying on the terrace
    results["torus"] = r.voxelize_triangles(tv, tf, color=(230, 150, 60), mat=54, reset=False, **dict(zip(("lo", "hi"), r.mesh_box(tv))))
    sv, sf = icosphere((0.3 * dx, -18.2 * dx, 0.4 * dx), 9.4 * dx, 3)              # a glowing ball in the torus's hole
    shade = (200 + 55 * (sv[sf].mean(axis=1)[:, 1] - sv[:, 1].min()) / np.ptp(sv[:, 1])).astype(int)   # one colour a triangle
    results["sphere"] = r.voxelize_triangles(sv, sf, color=np.stack([shade, shade * 3 // 5, shade // 4], axis=1), mat=2, reset=False,
                                             **dict(zip(("lo", "hi"), r.mesh_box(sv))))
    cv, cf = icosphere((22.3 * dx, -24.0 * dx, 0.0), 6.2 * dx, 2)                  # a bite out of the torus: mat = 0 carves
    results["carve"] = r.voxelize_triangles(cv, cf, color=(0, 0, 0), mat=0, **dict(zip(("lo", "hi"), r.mesh_box(cv))))
    for name, res in results.items():
        print(f"{name}: {int(res['voxels'])} voxels written in {res['lo'].tolist()} .. {res['hi'].tolist()}, {int(res['invalid'])} invalid triangles")
    for _ in range(frames):
        r.accumulate(spp)
    r.session.sync()
    out = os.environ.get("VRT_OUT", os.path.join("screenshot", "voxelize_mesh.png"))
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        save_image(r.fetch_image(), out)
        print(f"Image has been saved to {out}")
    return r, results


if __name__ == "__main__":
    main()
