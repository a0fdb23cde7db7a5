"""How fast vrt_gather_probes answers, next to the way the same numbers were to be had before it existed: probes/s on one GPU, in one
process.

    python tools/probe_rate.py [--reps 9] [--warmup 3] [--probes 4096] [--samples 64] [--depth 8] [--out profiles/probe_rate.jsonl]

`--probes` probes on the headline scene S1 -- the centres of empty cells around and above its voxels (Renderer.probe_lattice's rule, on
the scene's arrays) -- `--samples` samples a probe at `--depth` bounces.  Wall clock from host arrays to host records, the median of
--reps repetitions after --warmup with the 10th and 90th percentile, of two ways:
  gather   Renderer-style host path: one vrt_gather_probes call over the probes (16 bytes a probe in, 128 bytes a probe back);
  host     directions drawn on the host (numpy: uniform on the sphere), one vrt_path_ray per (probe, sample) through vrt_trace_radiance's
           host path at one sample a ray, and the projection onto the nine basis functions in numpy.  This way has no separate sun: the
           disc is met by chance, so its coefficients are noisier than the gather's at the same sample count -- the rates compare the
           cost, not the quality.
Also the gather on the device path (records resident, wall clock around a sync), which has no counterpart.  Prints one JSON line and
appends it to --out."""
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


def probes_of(mat, n):
    st = VoxelStore()
    st._init_voxels(mat.shape[0])
    st.voxel_material[...] = mat
    solid = np.argwhere(mat > 0)
    g = mat.shape[0]
    lo, hi = np.maximum(solid.min(axis=0) - 8, 0), np.minimum(solid.max(axis=0) + 17, g)
    centre, _ = st.probe_lattice(lo, hi, 2)
    rng = np.random.default_rng(0)
    if len(centre) < n:
        raise SystemExit(f"the lattice holds {len(centre)} empty cells, fewer than --probes {n}")
    p = np.zeros(n, _abi.PROBE)
    p["pos"] = centre[np.sort(rng.choice(len(centre), n, replace=False))]
    p["stream"] = np.arange(n)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--probes", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--out", default=os.path.join("profiles", "probe_rate.jsonl"))
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
    probes = probes_of(mat, a.probes)
    n, spp = len(probes), a.samples
    keep = {}

    def gather():
        keep["gather"] = s.gather_probes(probes, spp, 0)

    def by_host():
        rng = np.random.default_rng(1)
        v = rng.normal(size=(n * spp, 3))
        w = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
        rays = np.zeros(n * spp, _abi.PATH_RAY)
        rays["origin"], rays["dir"], rays["stream"] = np.repeat(probes["pos"], spp, axis=0), w, np.arange(n * spp)
        L = s.trace_radiance(rays, 1, 0)["rgb"].astype(np.float64)
        Y = VoxelStore.sh_basis(w)
        keep["host"] = (4.0 * np.pi / spp) * np.einsum("ksi,ksc->kic", Y.reshape(n, spp, 9), L.reshape(n, spp, 3))

    t_in = torch.from_numpy(probes.view(np.uint8).reshape(-1)).cuda()
    t_out = torch.zeros(n * 32, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    g = timed(gather, lambda: None, a.reps, a.warmup)
    h = timed(by_host, lambda: None, a.reps, a.warmup)
    d = timed(lambda: s.gather_probes(t_in, spp, 0, t_out), s.sync, a.reps, a.warmup)
    rec = keep["gather"]
    row = dict(tool="probe_rate", build=_lib.build_id(), scene="s1", probes=n, samples=spp, depth=a.depth, items=n * spp,
               gather_ms=g[0] * 1e3, gather_p10_ms=g[1] * 1e3, gather_p90_ms=g[2] * 1e3, gather_probes_per_s=n / g[0],
               host_ms=h[0] * 1e3, host_p10_ms=h[1] * 1e3, host_p90_ms=h[2] * 1e3, host_probes_per_s=n / h[0],
               device_path_ms=d[0] * 1e3, device_path_p10_ms=d[1] * 1e3, device_path_p90_ms=d[2] * 1e3, device_path_probes_per_s=n / d[0],
               ratio_gather_to_host=h[0] / g[0], mean_sky=float(rec["sky"].mean()), mean_sun=float(rec["sun"].mean()),
               mean_sh0=[float(x) for x in rec["sh"][:, 0].mean(axis=0)], host_mean_sh0=[float(x) for x in keep["host"][:, 0].mean(axis=0)])
    s.close()
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
