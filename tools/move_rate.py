"""What vrt_move_voxels costs, next to the edit it ends in and next to today's device route for a translation: milliseconds a call on one
GPU, in one process.

    python tools/move_rate.py [--reps 9] [--warmup 2] [--out profiles/move_rate.jsonl]

Wall clock around the call and the wait for the context's stream; the box's voxels are put back (untimed) before every repetition, so
every repetition moves the same voxels.  On the sparse headline scene S1 and on the half-full `dense` at 128^3, for a 64^3 box at the
grid's centre and for the whole grid; and on the whole grid of `sponge256` at 256^3; source box = destination box = that box; all in the
same run:
  (a) vrt_update_voxels of the box with its own content (device path): the floor the call ends in, once per box it edits;
  (b) today's device route for a translation: vrt_fetch_voxels + torch.roll / torch.where + vrt_update_voxels;
  (c) vrt_move_voxels by the identity, by a translation of (3, 2, 1), by a quarter turn and by a 30 degree turn about z through the box's
      centre, each as a copy and with VRT_MOVE_ERASE_SOURCE;
  (d) the same with VRT_MOVE_DRY_RUN.
Each figure is the median of --reps repetitions after --warmup, with the 10th and 90th percentile.  One JSON line per configuration is
printed and appended to --out; `ratios` lines hold (c)/(a), (c)/(b) (translation only) and (c)/(c identity)."""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voxel_rt2_amd import _abi, _lib, host, materials, scenes  # noqa: E402
from voxel_rt2_amd._session import NativeSession  # noqa: E402
from voxel_rt2_amd.renderer import Renderer  # noqa: E402


def timed(fn, sync, restore, reps, warmup):
    out = []
    for k in range(warmup + reps):
        restore()
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if k >= warmup:
            out.append(time.perf_counter() - t0)
    out.sort()
    return statistics.median(out), out[len(out) // 10], out[(9 * len(out)) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "move_rate.jsonl"))
    ap.add_argument("--scenes", default="s1,dense,sponge256")
    a = ap.parse_args()
    import torch
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    today = datetime.date.today().isoformat()

    def emit(**row):
        row = dict(tool="move_rate", build=_lib.build_id(), date=today, **row)
        line = json.dumps(row)
        print(line, flush=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")

    def ms(t):
        return dict(ms=t[0] * 1e3, p10_ms=t[1] * 1e3, p90_ms=t[2] * 1e3)
    for scene, edges in (("s1", (64, 128)), ("dense", (64, 128)), ("sponge256", (256,))):
        if scene not in a.scenes.split(","):
            continue
        mat, rgb, params = scenes.SCENES[scene](0)
        G = mat.shape[0]
        s = NativeSession(_lib.load(), "vrt_", host.make_config(64, 64, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=2, grid_res=G))
        s.upload_voxels(mat, rgb)
        s.upload_materials(materials.load_table())
        s.set_scene(host.make_scene_params(**params))
        s.set_camera(host.default_camera(64, 64))
        s.prepare()
        for edge in edges:
            lo = ((G - edge) // 2,) * 3
            hi = tuple(l + edge for l in lo)
            sl = tuple(slice(l, h) for l, h in zip(lo, hi))
            keep_m, keep_c = torch.from_numpy(mat[sl].copy()).cuda(), torch.from_numpy(rgb[sl].copy()).cuda()
            bm, bc = torch.empty_like(keep_m), torch.empty_like(keep_c)
            torch.cuda.synchronize()
            restore = lambda: s.update_voxels(lo, hi, keep_m.data_ptr(), keep_c.data_ptr(), on_device=True)
            nothing = lambda: None
            t_a = timed(restore, s.sync, nothing, a.reps, a.warmup)
            emit(what="a_update_voxels", scene=scene, grid_res=G, box=edge, **ms(t_a))
            shift = (3, 2, 1)

            def today_route():
                s.fetch_voxels(lo, hi, bm.data_ptr(), bc.data_ptr(), on_device=True)
                s.sync()                                                    # torch's stream reads what the context's stream wrote
                here = torch.zeros_like(bm, dtype=torch.bool)
                here[shift[0]:, shift[1]:, shift[2]:] = (bm > 0)[:edge - shift[0], :edge - shift[1], :edge - shift[2]]
                rm, rc = torch.roll(bm, shift, (0, 1, 2)), torch.roll(bc, shift, (0, 1, 2))
                out_m = torch.where(here, rm, torch.where(bm > 0, torch.zeros_like(bm), bm))
                out_c = torch.where(here[..., None], rc, torch.where((bm > 0)[..., None], torch.zeros_like(bc), bc))
                torch.cuda.synchronize()
                s.update_voxels(lo, hi, out_m.data_ptr(), out_c.data_ptr(), on_device=True)
                s.sync()                                                    # (out_m, out_c are torch's: freed when this returns)
            t_b = timed(today_route, s.sync, restore, a.reps, a.warmup)
            emit(what="b_fetch_where_update", scene=scene, grid_res=G, box=edge, **ms(t_b))
            centre = tuple((l + h) / 2 for l, h in zip(lo, hi))
            maps = (("identity", None, None, (0, 0, 0)), ("translation", None, None, shift), ("turn90", Renderer.rotation_matrix("z", 90), centre, (0, 0, 0)),
                    ("turn30", Renderer.rotation_matrix("z", 30), centre, (0, 0, 0)))
            base = {}
            for name, rot, pivot, sh in maps:
                m, t = Renderer.move_transform(rot, pivot, sh)
                for dry in (False, True):
                    for erase in (False, True):
                        flags = (_abi.MOVE_ERASE_SOURCE if erase else 0) | (_abi.MOVE_DRY_RUN if dry else 0)
                        got = {}

                        def call():
                            got.update(s.move_voxels(lo, hi, lo, hi, m, t, flags))
                        restore()                                           # (a dry run changes nothing: once is enough)
                        t_c = timed(call, s.sync, nothing if dry else restore, a.reps, a.warmup)
                        emit(what="d_move_dry_run" if dry else "c_move", scene=scene, grid_res=G, box=edge, map=name, erase=erase, written=got["written"],
                             blocked=got["blocked"], erased=got["erased"], voxels_per_s=edge ** 3 / t_c[0], **ms(t_c))
                        if name == "identity":
                            base[(dry, erase)] = t_c[0]
                        ratios = dict(c_over_a=t_c[0] / t_a[0], c_over_identity=t_c[0] / base[(dry, erase)])
                        if name == "translation" and erase and not dry:
                            ratios["c_over_b"] = t_c[0] / t_b[0]
                        emit(what="ratios", scene=scene, grid_res=G, box=edge, map=name, erase=erase, dry_run=dry, **ratios)
            del keep_m, keep_c, bm, bc
        s.close()


if __name__ == "__main__":
    main()
