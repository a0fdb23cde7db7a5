"""The reference's example scripts run UNMODIFIED against this repo's `scene.py` + host-side `taichi`
module.  On this CPU-only box the GPU renderer is replaced by a recorder that keeps
the voxel grid the script authors, so what is tested is the Scene API surface and the DSL shim.  The scripts
are read from the reference tree at test time (never copied); without it the tests that run them skip.
Every run is also compared EXACTLY with tests/golden/examples.json (sha256 of the authored voxel arrays and every scene
parameter, written by tests/golden/make_example_fixtures.py): a voxel that moves fails the hash, not just a range.

The shim computes kernels in binary32 / int32 like Taichi (taichi/_kernel.py), in plain Python: the eleven scripts take three
minutes of CPU between them (example5 alone loops over 12 M cells), so they run ONCE per session, as parallel processes
(`example_runs`), and the tests below look at what they left."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


from voxel_rt2_amd.renderer import VoxelStore, _Field, _AtmosProxy  # noqa: E402


class RecorderRenderer(VoxelStore):
    """Stands in for voxel_rt2_amd.renderer.Renderer: same surface and voxel store, no GPU."""
    instances = []

    def __init__(self, dx, image_res, up, voxel_edges, exposure=3, **kw):
        self.args = dict(dx=dx, image_res=image_res, voxel_edges=voxel_edges, exposure=exposure)
        self._init_voxels()
        self.floor_height, self.floor_color, self.floor_material = _Field(0.0), _Field((1, 1, 1)), _Field(1)
        self.background_color, self.use_physical_atmosphere = _Field((0, 0, 0)), _Field(0)
        self.atmos = _AtmosProxy(None)
        self.fov = _Field(float(np.deg2rad(50.0)))
        self.light = None
        self.calls = []
        RecorderRenderer.instances.append(self)

    def set_directional_light(self, direction, cone, color):
        self.light = (tuple(direction), cone, tuple(color))

    def set_camera_pos(self, *a): self.calls.append("set_camera_pos")
    def prepare_data(self): self.calls.append("prepare_data")


FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "examples.json")))
SCRIPTS = ["main.py"] + [f"example{i}.py" for i in range(1, 11)]


class Run:
    def __init__(self, outdir, name):
        self.d = json.load(open(os.path.join(outdir, name + ".json")))
        a = np.load(os.path.join(outdir, name + ".npz"))
        self.voxel_material, self.voxel_color = a["voxel_material"], a["voxel_color"]
        self.calls = self.d.pop("calls")


@pytest.fixture(scope="session")
def example_runs(tmp_path_factory):
    if not os.path.isdir(REF):
        pytest.skip("the reference's example scripts are read from the reference tree, which is not present")
    out = str(tmp_path_factory.mktemp("examples"))
    gen = os.path.join(ROOT, "tests", "golden", "make_example_fixtures.py")
    procs = {n: subprocess.Popen([sys.executable, gen, "--record", n, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for n in SCRIPTS}
    logs = {n: p.communicate(timeout=900)[0] for n, p in procs.items()}
    bad = {n: logs[n][-2000:] for n, p in procs.items() if p.returncode != 0}
    assert not bad, bad
    return {n: Run(out, n) for n in SCRIPTS}


@pytest.mark.parametrize("name", SCRIPTS)
def test_script_authors_the_grid_and_parameters_of_the_fixture(name, example_runs):
    got, want = example_runs[name].d, FIXTURE[name]
    assert got == want, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}
    assert example_runs[name].calls[-1] == "prepare_data"


def test_example6_grid_fixture_is_the_scripts_grid(example_runs):
    """tests/golden/example6_grid.npz (what the GPU box renders in place of the script, tests/test_gpu_parity.py) holds exactly
    the arrays example6.py authors."""
    r = example_runs["example6.py"]
    g = np.load(os.path.join(ROOT, "tests", "golden", "example6_grid.npz"))
    assert np.array_equal(g["voxel_material"], r.voxel_material) and np.array_equal(g["voxel_color"], r.voxel_color)


def test_example1(example_runs):
    r = example_runs["example1.py"]
    m = r.voxel_material
    assert r.d["exposure"] == 10 and r.d["floor_height"] == -0.05
    assert (m[64:114, 64, 64:114] > 0).all()                      # the 50 x 50 slab at y = 0
    assert (m[64, 64, 64:114] == 2).all() and (m[65:113, 64, 65:113] == 1).all()
    assert tuple(r.voxel_color[70, 64, 70]) == (229, 25, 25)       # trunc(0.9*255), trunc(0.1*255)
    towers = (m[:, 65:, :] > 0).sum()
    assert 200 < towers < 2500 and (m[:, 65:, :] == 2).sum() > 30  # ~4 % of cells grow a capped tower
    assert r.d["light"] == dict(direction=[1.0, 1.0, 1.0], cone=0.1, color=[0.0, 0.0, 0.0])   # default sun (scene.py:127)


def test_example4_sphere(example_runs):
    r = example_runs["example4.py"]
    solid = (r.voxel_material > 0)
    vol = 4 / 3 * np.pi * (60 * np.sqrt(0.5)) ** 3
    assert abs(solid.sum() - vol) / vol < 0.02
    assert r.d["light"]["color"] == [1, 1, 1] and r.d["background_color"] == [0.3, 0.4, 0.6]


@pytest.mark.parametrize("name,lo,hi", [("main.py", 1, 1), ("example2.py", 1500, 3000), ("example3.py", 9000, 16000),
                                         ("example5.py", 20000, 400000),
                                         ("example8.py", 150000, 500000), ("example10.py", 50000, 250000)])
def test_example_fills_grid(name, lo, hi, example_runs):
    n = int((example_runs[name].voxel_material != 0).sum())
    assert lo <= n <= hi, n


def test_example6_scene_parameters(example_runs):
    r = example_runs["example6.py"]
    assert 100000 <= int((r.voxel_material != 0).sum()) <= 400000
    assert r.d["use_physical_sky"] == 1 and r.d["use_clouds"] == 1
    assert r.d["voxel_edges"] == 0 and r.d["exposure"] == 2.0 and r.d["floor_height"] == -0.85
    np.testing.assert_allclose(r.d["light"]["color"], (1.3, 0.949 * 1.3, 0.937 * 1.3))
    assert set(np.unique(r.voxel_material)) <= {0, 11, 80}


@pytest.mark.parametrize("name", ["example7.py", "example9.py"])
def test_heavy_dsl_examples(name, example_runs):
    """example7 (swizzles, int()/float()/any() on vectors, 78 kernel launches) and example9 (default vector
    arguments, get_voxel round trips, float material ids)."""
    r = example_runs[name]
    n = int((r.voxel_material != 0).sum())
    assert n > 50000, n
    if name == "example7.py":
        assert r.d["floor_material"] == 20 and r.d["use_physical_sky"] == 1
        assert {10, 11}.issubset(set(np.unique(r.voxel_material)))
    else:
        assert r.d["voxel_edges"] == 0 and r.d["exposure"] == 2.75
        assert (r.voxel_material == 2).sum() > 1000  # the ceiling light strip


def test_shim_equals_the_independent_reading_of_taichi_on_short_scripts(tmp_path, example_runs):
    """tools/refexec_examples: the same scripts under tests/refexec -- the emulation of Taichi the reference vectors are made with,
    written independently of the product's shim -- with the reference's OWN Scene class, the same random stream and elementary
    functions: identical voxel arrays.  Two short scripts here (seconds); `bash tools/refexec_examples/check_all.sh` does all
    eleven (minutes; round 4: all identical)."""
    for name in ("example2.py", "example3.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "refexec_examples", "run.py"), name], capture_output=True, text=True,
                           timeout=600, env=dict(os.environ, REFEXEC_EXAMPLES_OUT=str(tmp_path)), cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        e = np.load(os.path.join(str(tmp_path), name + ".npz"))
        assert np.array_equal(e["m"], example_runs[name].voxel_material) and np.array_equal(e["c"], example_runs[name].voxel_color), name


def test_kernel_scope_is_binary32():
    """The rules the shim stands for, on kernels small enough to work out by hand (taichi/_kernel.py)."""
    import struct
    import taichi as ti
    from taichi.math import vec3
    f32 = lambda x: struct.unpack("f", struct.pack("f", x))[0]  # noqa: E731
    out = {}

    @ti.kernel
    def k():
        for i in range(3, 4):
            out["index product"] = 0.5 - i * 0.1            # f32(0.5 - f32(3 * f32(0.1))), not the double expression rounded once
        a = 1
        a = 2.75                                            # an i32 variable: the float truncates
        out["typed local"] = a
        p = ti.max(-1.5, 0)                                 # f32 beside an integer: an f32 zero ...
        p = 0.25                                            # ... so this does not truncate
        out["max promotes"] = p
        out["int division"] = 7 / 2                         # true division in default_fp
        out["floor division"] = -7 // 2
        out["round"] = (ti.round(2.5), ti.round(-2.5), int(-2.7))      # half away from zero; int() truncates
        out["vector"] = (vec3(0.1, 0.2, 0.3) * 3).to_list()
        out["pow"] = 1.1 ** 3                               # x * x * x in f32
    k()
    assert out["index product"] == f32(f32(0.5) - f32(3 * f32(0.1))) and out["index product"] != f32(0.5 - 3 * 0.1)
    assert out["typed local"] == 2 and isinstance(out["typed local"], int)
    assert out["max promotes"] == 0.25
    assert out["int division"] == 3.5 and out["floor division"] == -4
    assert out["round"] == (3.0, -3.0, -2)
    assert out["vector"] == [f32(f32(0.1) * 3), f32(f32(0.2) * 3), f32(f32(0.3) * 3)]
    x = f32(1.1)
    assert out["pow"] == f32(x * f32(x * x))
    # module-level code of a script is plain Python: doubles
    assert (vec3(0.1, 0.2, 0.3) * 3).to_list() == [0.1 * 3, 0.2 * 3, 0.3 * 3]
