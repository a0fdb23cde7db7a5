"""The shading point of a pixel's primary vertex built once for all fused samples (csrc/vrt_primary.h primary_vertex_surf, handed to
primary_vertex_sample and through it to path_shade<..., SURF_GIVEN>; csrc/vrt_path.h path_surf) against the form that builds it per
sample, on the host build of the device headers, without a GPU.  tests/emul/primary_shared_emul.cpp runs every pixel of a frame and samples
0-3 through both forms and counts what differs: the words of the shading point (as uint32, field by field), the words of every path that
goes on (its continuation record and the fields the record leaves out), and the bytes of the colour and reflection-depth planes the
finished paths stored.  All three counts are 0.

The same loop goes through a stand-alone program built with -fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orc
from voxel_rt2_amd import host, materials, scenes
from voxel_rt2_amd._session import NativeSession

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_primary_shared_emul.so")
_SRC = os.path.join(HERE, "emul", "primary_shared_emul.cpp")
HOST_FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wno-unknown-pragmas"]   # (emu.build's)
CASES = {"s1_64x64_d4": ("s1", 64, 64, 4), "sunlit_80x48_d6": ("sunlit", 80, 48, 6)}   # scene, W, H, depth
SAMPLES = 4


@pytest.fixture(scope="module")
def lib():
    csrc, inc = os.path.join(ROOT, "voxel_rt2_amd", "csrc"), os.path.join(ROOT, "include")
    deps = ([os.path.join(HERE, "emul", f) for f in ("primary_shared_emul.cpp", "primary_vertex_emul.cpp", "emul.cpp")] +
            [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")] + [os.path.join(inc, f) for f in os.listdir(inc)])
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.run(["g++", "-O2", "-fPIC", "-shared"] + HOST_FLAGS + ["-o", _SO, _SRC], check=True, capture_output=True)
    so = C.CDLL(_SO)
    so.emu_primary_shared_check.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]
    return so


def _setup(case):
    scene, W, H, depth = CASES[case]
    mat, rgb, params = scenes.SCENES[scene](0)
    params = dict(params, use_physical_sky=0, use_clouds=0)   # (the sky tables are test_emul_parity's)
    cfg = host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=depth, seed=3)
    return cfg, mat, rgb, params


@pytest.mark.parametrize("case", sorted(CASES))
def test_shared_shading_point_leaves_every_sample_as_the_per_sample_form_does(lib, case):
    cfg, mat, rgb, params = _setup(case)
    e = NativeSession(lib, "emu_", cfg)
    orc.setup(e, mat, rgb, params)
    counts = (C.c_ulonglong * 6)()
    assert lib.emu_primary_shared_check(C.c_void_p(e._ctx), SAMPLES, 1, counts) == 0
    e.close()
    surfaces, samples, sent_on, surf_words, path_words, plane_bytes = (int(x) for x in counts)
    print(f"{case}: {surfaces} pixels with a shading point, {samples} pixel-samples, {sent_on} sent on; differing: shading-point words {surf_words}, "
          f"path words {path_words}, plane bytes {plane_bytes}")
    assert samples == cfg.width * cfg.height * SAMPLES
    assert 0 < surfaces <= cfg.width * cfg.height and 0 < sent_on < samples   # surfaces and ends, paths that go on and paths that do not
    assert surf_words == 0
    assert path_words == 0
    assert plane_bytes == 0


def test_sanitized_stand_alone_program(tmp_path):
    """The same loop under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own."""
    exe = str(tmp_path / "primary_shared_main")
    subprocess.run(["g++", "-O1", "-g", "-DPRIMARY_SHARED_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"] +
                   HOST_FLAGS + ["-o", exe, _SRC], check=True, capture_output=True)
    for case in sorted(CASES):
        cfg, mat, rgb, params = _setup(case)
        path = str(tmp_path / f"{case}.case")
        with open(path, "wb") as f:
            f.write(bytes(cfg))
            f.write(bytes(host.make_scene_params(**params)))
            f.write(bytes(host.default_camera(cfg.width, cfg.height)))
            f.write(np.uint32(SAMPLES).tobytes())
            f.write(np.ascontiguousarray(mat, dtype=np.int8).tobytes())
            f.write(np.ascontiguousarray(rgb, dtype=np.uint8).tobytes())
            f.write(np.ascontiguousarray(materials.load_table(), dtype=np.float32).tobytes())
        r = subprocess.run([exe, path], capture_output=True, text=True)
        print(case, r.stdout.strip())
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
        assert r.stdout.strip().endswith("of the paths 0, bytes of the planes 0") and "shading point that differ 0," in r.stdout
