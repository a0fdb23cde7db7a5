"""How fast vrt_gather_irradiance answers, next to vrt_trace_radiance on the same number of items: items/s on one GPU, in one process.

    python tools/sensor_rate.py [--reps 9] [--warmup 3] [--samples 16] [--depth 8] [--out profiles/sensor_rate.jsonl]

2^18 sensors on the headline scene S1 -- the exposed faces of its voxels (Renderer.surface_faces' rule, on the scene's arrays) filled up
with floor points around the slab -- device resident, `--samples` samples a sensor at `--depth` bounces through the device path: wall
clock around a sync, the median of --reps repetitions after --warmup with the 10th and 90th percentile.  Next to it, in the same
context, the same number of items through vrt_trace_radiance: one ray a sensor, from the sensor's origin along ONE cosine-distributed
direction around its normal drawn here on the host (the gather's own density, normal + a point of the unit sphere; along the normal
itself the paths would be shallower and escape more often than the gather's), the same number of samples.  The query's samples of a
sensor share that direction where the gather draws one per sample: over 2^18 sensors the two loads have the same distribution of
first segments, not the same rays.  An item of a gather is an item of that query plus one shadow walk, so the gather's rate is expected
below the query's measured here by about the share of walks added.  Prints one JSON line and appends it to --out."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voxel_rt2_amd import _abi, _lib, host, materials, scenes  # noqa: E402
from voxel_rt2_amd._session import NativeSession  # noqa: E402
from voxel_rt2_amd.renderer import VoxelStore  # noqa: E402
from radiance_rate import timed  # noqa: E402

N = 1 << 18


def sensors_of(mat, floor_height):
    st = VoxelStore()
    st._init_voxels(mat.shape[0])
    st.voxel_material[...] = mat
    cell, face, centre, normal = st.surface_faces()
    rng = np.random.default_rng(0)
    if len(centre) > N:
        keep = np.sort(rng.choice(len(centre), N, replace=False))
        centre, normal = centre[keep], normal[keep]
    fill = N - len(centre)
    solid = np.argwhere(mat > 0)
    g = mat.shape[0]
    lo, hi = (solid.min(axis=0) - 8 - g / 2) * (2.0 / g), (solid.max(axis=0) + 9 - g / 2) * (2.0 / g)
    pts = np.stack([rng.uniform(lo[0], hi[0], fill), np.full(fill, floor_height), rng.uniform(lo[2], hi[2], fill)], axis=1)
    s = np.zeros(N, _abi.SENSOR)
    s["pos"] = np.concatenate([centre, pts.astype(np.float32)])
    s["normal"] = np.concatenate([normal, np.tile(np.float32((0.0, 1.0, 0.0)), (fill, 1))])
    s["stream"] = np.arange(N)
    return s, N - fill


def hemisphere_dirs(normal, rng):
    """One cosine-distributed direction around each unit normal: normal + a uniform point of the unit sphere, normalised (vrt_bsdf.h's
    cosine_dir, with numpy's draws)."""
    v = rng.normal(size=normal.shape)
    w = normal + v / np.linalg.norm(v, axis=1, keepdims=True) * (1.0 - 1e-5)
    return (w / np.linalg.norm(w, axis=1, keepdims=True)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--out", default=os.path.join("profiles", "sensor_rate.jsonl"))
    a = ap.parse_args()
    import torch
    mat, rgb, params = scenes.SCENES["s1"](0)
    s = NativeSession(_lib.load(), "vrt_", host.make_config(64, 32, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=a.depth,
                                                            grid_res=mat.shape[0]))
    s.upload_voxels(mat, rgb)
    s.upload_materials(materials.load_table())
    s.set_scene(host.make_scene_params(**params))
    s.set_camera(host.default_camera(64, 32))
    s.prepare()
    sensors, n_faces = sensors_of(mat, params["floor_height"])
    rays = np.zeros(N, _abi.PATH_RAY)
    rays["origin"], rays["stream"] = sensors["pos"] + sensors["normal"] * np.float32(1e-6), sensors["stream"]
    rays["dir"] = hemisphere_dirs(sensors["normal"], np.random.default_rng(1))
    t_sensors = torch.from_numpy(sensors.view(np.uint8).reshape(-1)).cuda()
    t_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
    t_irr = torch.zeros(N * 8, dtype=torch.float32, device="cuda")
    t_rad = torch.zeros(N * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    items = N * a.samples
    g = timed(lambda: s.gather_irradiance(t_sensors, a.samples, 0, t_irr), s.sync, a.reps, a.warmup)
    q = timed(lambda: s.trace_radiance(t_rays, a.samples, 0, t_rad), s.sync, a.reps, a.warmup)
    irr = t_irr.view(-1, 8).mean(dim=0).cpu()
    row = dict(tool="sensor_rate", build=_lib.build_id(), radiance_rays="one host-drawn cosine-distributed direction a sensor", scene="s1", sensors=N, faces=int(n_faces), samples=a.samples, depth=a.depth, items=items,
               gather_ms=g[0] * 1e3, gather_p10_ms=g[1] * 1e3, gather_p90_ms=g[2] * 1e3, gather_items_per_s=items / g[0],
               radiance_ms=q[0] * 1e3, radiance_p10_ms=q[1] * 1e3, radiance_p90_ms=q[2] * 1e3, radiance_items_per_s=items / q[0],
               ratio_gather_to_radiance=q[0] / g[0], mean_sky=float(irr[3]), mean_sun=float(irr[7]), mean_sky_rgb=[float(x) for x in irr[:3]])
    s.close()
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
