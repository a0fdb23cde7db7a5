"""Solids from triangle meshes on the terrace of moving_box.py: the torus and the icosphere of voxelize_mesh.py, this time FILLED
(Renderer.fill_triangles -> vrt_fill_triangles: every voxel whose centre lies inside the closed mesh), the torus with its conservative
skin on top (shell=True), and a bite carved out of the torus as a volume: a smaller sphere filled with mat = 0.  Where the bite cuts
the torus the cut shows solid material, not an eggshell.  Headless; new code, not one of the reference's scripts.  Run from the repo root:

    VRT_RES=640x360 VRT_FRAMES=16 VRT_SPP=4 VRT_SKY_RES=512 python examples/fill_mesh.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from scene import Scene, save_image  # noqa: E402
from voxelize_mesh import icosphere, torus  # noqa: E402


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
    tv, tf = torus((0.0, -26.5 * dx, 0.0), 22.3 * dx, 7.6 * dx)                    # lying on the terrace: solid, with its skin
    results["torus"] = r.fill_triangles(tv, tf, color=(230, 150, 60), mat=54, shell=True, reset=False)
    sv, sf = icosphere((0.3 * dx, -18.2 * dx, 0.4 * dx), 9.4 * dx, 3)              # a glowing ball in the torus's hole: solid
    results["sphere"] = r.fill_triangles(sv, sf, color=(255, 160, 70), mat=2, reset=False)
    cv, cf = icosphere((22.3 * dx, -24.0 * dx, 0.0), 6.2 * dx, 2)                  # a bite out of the torus: a filled mesh with mat = 0
    results["carve"] = r.fill_triangles(cv, cf, color=(0, 0, 0), mat=0)
    for name, res in results.items():
        print(f"{name}: {int(res['voxels'])} voxels written in {res['lo'].tolist()} .. {res['hi'].tolist()}, {int(res['invalid'])} invalid triangles")
    for _ in range(frames):
        r.accumulate(spp)
    r.session.sync()
    out = os.environ.get("VRT_OUT", os.path.join("screenshot", "fill_mesh.png"))
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        save_image(r.fetch_image(), out)
        print(f"Image has been saved to {out}")
    return r, results


if __name__ == "__main__":
    main()
