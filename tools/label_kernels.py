"""Where a vrt_label_components call spends its time: the three kernels' durations per configuration, from a kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/label_kernels.py run
    python tools/label_kernels.py digest DIR [profiles/label_kernels.jsonl]

`run` makes a known sequence of whole-grid calls on the device path (CONFIGS x REPS, a wait after each); `digest` needs no GPU: it
picks the k_label_* dispatches out of the trace in time order, cuts them into calls at every k_label_tile, and writes per configuration
the median duration of each kernel and of the span from the first kernel's start to the last one's end, the first repetition left out."""
import csv
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = [("s1", 6, True), ("s1", 26, True), ("dense", 6, False), ("dense", 26, False), ("sponge256", 6, False), ("sponge256", 6, True), ("sponge256", 26, True)]
REPS = 6


def run():
    import torch
    from voxel_rt2_amd import _lib, host, materials, scenes
    from voxel_rt2_amd._session import NativeSession
    s, open_scene = None, None
    for scene, conn, empty in CONFIGS:
        if scene != open_scene:
            if s is not None:
                s.close()
            mat, rgb, params = scenes.SCENES[scene](0)
            s = NativeSession(_lib.load(), "vrt_", host.make_config(64, 64, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=2, grid_res=mat.shape[0]))
            s.upload_voxels(mat, rgb)
            s.upload_materials(materials.load_table())
            s.set_scene(host.make_scene_params(**params))
            s.set_camera(host.default_camera(64, 64))
            s.prepare()
            open_scene, G = scene, mat.shape[0]
        labels = torch.empty((G, G, G), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(REPS):
            s.label_components((0, 0, 0), (G, G, G), conn, empty, out=labels)
            s.sync()
        del labels
    s.close()


def digest(d, out):
    ev = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "k_label" in r["Kernel_Name"]:
                ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].split("::")[-1]))
    ev.sort()
    calls = []
    for e in ev:
        if "k_label_tile" in e[2]:
            calls.append([])
        calls[-1].append(e)
    assert len(calls) == len(CONFIGS) * REPS, (len(calls), len(ev))
    with open(out, "w") as fh:
        for i, (scene, conn, empty) in enumerate(CONFIGS):
            mine = calls[i * REPS + 1:(i + 1) * REPS]
            row = dict(scene=scene, connectivity=conn, members="empty" if empty else "solid")
            for k in range(3):
                row[mine[0][k][2] + "_us"] = statistics.median((c[k][1] - c[k][0]) / 1e3 for c in mine)
            row["span_us"] = statistics.median((c[-1][1] - c[0][0]) / 1e3 for c in mine)
            fh.write(json.dumps(row) + "\n")
            print(json.dumps(row))


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["digest"]:
        digest(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else os.path.join("profiles", "label_kernels.jsonl"))
    else:
        sys.exit(__doc__)
