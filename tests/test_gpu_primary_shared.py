"""k_primary_vertex builds the shading point of a pixel's primary vertex once for all fused samples of a launch (csrc/vrt_primary.h
primary_vertex_surf, handed to path_shade<..., SURF_GIVEN>).  That changes no bit of what a context renders: the HDR frame, both histories
and g-buffer depth / normal / material / position of every case are those of the same calls rendered with VRT_PRIMARY=0, where the pool
builds the shading point per sample.  The cases are the ones tests/test_gpu_primary_vertex.py does not reach:

  s6 under the physical sky (tables precomputed as test_sky_precompute_split_by_columns_on_the_gpu does): an escaped camera ray draws from
      its sample's random stream in sky_lookup, so escaped pixels have to stay per sample;
  sunlit with its non-zero plain background: every lobe at depth 0, the emitting sun's light sample with the shared shading point, and
      escapes that draw nothing;
  s1 on rows 5-43 of 96x56: emissive primary hits, which get no shading point, beside surfaces in one tile.

As there: every GPU run is a process of its own under `timeout`, on the development build, with VRT_FULL_BELOW=0 and four hardware queues;
every fused launch must be reported as served."""
import os
import re
import shlex
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CALLS = (4, 2, 3, 4)
# name: (scene, width, height, depth, rows or None, sky_res)
CASES = {
    "s6_sky_64x40": ("s6", 64, 40, 3, None, 96),
    "sunlit_80x48": ("sunlit", 80, 48, 6, None, 0),
    "s1_96x56_rows_5_43": ("s1", 96, 56, 4, (5, 43), 0),
}
KNOBS = ("VRT_OVERLAP", "VRT_STREAMS", "VRT_PASS_STREAM", "VRT_GRID_DIV", "VRT_DEFER", "VRT_CTX_LANE", "VRT_TEST_FAIL_LAUNCH", "VRT_DEEP_ITEMS",
         "VRT_DEEPER_ITEMS", "VRT_DRAIN_GATE", "VRT_PREPASS", "VRT_PREPASS_REPORT", "VRT_FULL_BELOW", "VRT_PRIMARY", "VRT_PRIMARY_CAP", "VRT_PRIMARY_REPORT")
BUFFERS = ("hist_d", "hist_s", "depth", "normal", "mat", "pos")


def _child(out_dir):
    """Every case in this process (the environment carries the switches); the state of each goes to out_dir/<case>.npz."""
    import orc
    from voxel_rt2_amd import _abi, _lib, host, scenes
    from voxel_rt2_amd._session import NativeSession
    lib = _lib.load_dev()
    which = dict(zip(BUFFERS, (_abi.BUF_HISTORY_DIFFUSE, _abi.BUF_HISTORY_SPECULAR, _abi.BUF_GBUF_DEPTH, _abi.BUF_GBUF_NORMAL, _abi.BUF_GBUF_MAT,
                               _abi.BUF_GBUF_POSITION)))
    for name, (scene, W, H, depth, rows, sky_res) in CASES.items():
        mat, rgb, params = scenes.SCENES[scene](0)
        sky = sky_res > 0
        assert bool(params["use_physical_sky"]) == sky
        if scene == "sunlit":
            assert any(x != 0.0 for x in params["background_color"]) and any(x != 0.0 for x in params["light_color"])
        cfg = host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=depth, seed=3, grid_res=mat.shape[0], sky_res=sky_res)
        if rows:
            cfg.row_begin, cfg.row_end = rows
        s = NativeSession(lib, "vrt_", cfg)
        orc.setup(s, mat, rgb, params, cloud=np.load(os.path.join(ROOT, "voxel_rt2_amd", "data", "cloud_texture.npy")) if sky else None)
        if sky:
            for _ in range(4):
                s.sky_accumulate_clouds(4)
            for sl in range(6):
                s.sky_compute_slice(sl, 6)
        for n in CALLS:
            s.accumulate(n)
        out = {"hdr": s.fetch_hdr()}
        for key, b in which.items():
            out[key] = s.fetch_buffer(b)
        print(f"case {name}:", flush=True)
        sys.stderr.flush()
        s.close()   # (the development build reports the context's served launches and path counts here, on stderr)
        np.savez(os.path.join(out_dir, name + ".npz"), **out)
    print("primary shared child: ok")


def _run(out_dir, primary):
    code = f"import os, sys; sys.path[:0] = [{ROOT!r}, os.path.join({ROOT!r}, 'tests')]; import test_gpu_primary_shared as t; t._child({str(out_dir)!r})"
    sets = {"VRT_PRIMARY": primary, "VRT_PRIMARY_REPORT": "1", "VRT_FULL_BELOW": "0", "GPU_MAX_HW_QUEUES": "4"}
    cmd = "env " + " ".join(f"{k}={shlex.quote(v)}" for k, v in sets.items()) + f" timeout -k 10 300 {shlex.quote(sys.executable)} -c {shlex.quote(code)}"
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run(["bash", "-c", cmd + " 2>&1"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0 and "primary shared child: ok" in r.stdout, r.stdout[-4000:]
    reports = {}
    for name, tail in re.findall(r"case (\S+):\n((?:(?!case ).*\n)*)", r.stdout):
        m = re.search(r"primary vertices served (\d+) of (\d+) render launches, paths finished (\d+) sent on (\d+)", tail)
        assert m, (name, tail)
        reports[name] = tuple(int(x) for x in m.groups())
    return reports


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    d = tmp_path_factory.mktemp("shared_off")
    reports = _run(d, "0")
    assert set(reports) == set(CASES) and all(r == (0, len(CALLS), 0, 0) for r in reports.values()), reports
    ref = {name: np.load(str(d / (name + ".npz"))) for name in CASES}
    for name, a in ref.items():   # pictures, not black frames
        assert np.isfinite(a["hdr"]).all() and a["hdr"].mean() > 0.0, name
    return ref


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("shared_on")
    reports = _run(d, "1")
    return reports, {name: np.load(str(d / (name + ".npz"))) for name in CASES}


@pytest.mark.parametrize("case", sorted(CASES))
def test_renders_what_the_pool_renders_with_a_shading_point_per_sample(case, run, reference):
    reports, got = run
    a, b = reference[case], got[case]
    served, launches, finished, sent_on = reports[case]
    print(f"{case}: served {served} of {launches} launches; paths finished {finished}, sent on {sent_on}")
    assert launches == len(CALLS)
    assert served == len(CALLS), "every launch is a fused one and is served"
    assert finished > 0 and sent_on > 0
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (case, k)
