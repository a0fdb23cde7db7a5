"""The primary-vertex stage (csrc/vrt_primary.h: what k_primary_vertex runs per pixel, and the BEGIN of the pooled launch behind it) on
the host build of the device headers, without a GPU.  tests/emul/primary_vertex_emul.cpp = emul.cpp plus emu_accumulate_primary: launches
of one sample each (sample index 0), a pixel at a time -- the wave's ballot compaction and samples 1-3 of a fused launch are the GPU
test's -- per tile and pixel the record, the hit, the g-buffer, primary_vertex_sample; continuations through the packed queue record
(primary_cont_pack, pool_begin_queued) into the emulated pool, leftovers through pool_begin_known / pool_begin.  The frames are the
oracle's bit for bit -- HDR, g-buffer, both histories -- with the queue the rule sizes, with eight records a head (nearly every
continuation takes the overflow route) and with every eleventh record spoilt (its pixel is left to the pool whole).

The same stage goes through a stand-alone program built with -fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orc
from voxel_rt2_amd import _abi, host, materials, scenes
from voxel_rt2_amd._session import NativeSession

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_primary_vertex_emul.so")
HOST_FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wno-unknown-pragmas"]   # (emu.build's)
BUFS = (_abi.BUF_GBUF_DEPTH, _abi.BUF_GBUF_NORMAL, _abi.BUF_GBUF_POSITION, _abi.BUF_GBUF_MAT, _abi.BUF_GBUF_REFL_DEPTH,
        _abi.BUF_HISTORY_DIFFUSE, _abi.BUF_HISTORY_SPECULAR)
CASES = {"s1_64x64_d4": ("s1", 64, 64, 4, 2), "sunlit_80x48_d6": ("sunlit", 80, 48, 6, 2)}   # scene, W, H, depth, samples
MODES = {"rule": (0, 0), "cap64": (64, 0), "cap64_spoilt": (64, 1)}                        # VRT_PRIMARY_CAP, spoil


@pytest.fixture(scope="module")
def lib():
    csrc, inc = os.path.join(ROOT, "voxel_rt2_amd", "csrc"), os.path.join(ROOT, "include")
    deps = ([os.path.join(HERE, "emul", f) for f in ("primary_vertex_emul.cpp", "emul.cpp")] +
            [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")] + [os.path.join(inc, f) for f in os.listdir(inc)])
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.run(["g++", "-O2", "-fPIC", "-shared"] + HOST_FLAGS + ["-o", _SO, os.path.join(HERE, "emul", "primary_vertex_emul.cpp")],
                       check=True, capture_output=True)
    so = C.CDLL(_SO)
    so.emu_accumulate_primary.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.POINTER(C.c_ulonglong)]
    return so


def _setup(case):
    scene, W, H, depth, spp = CASES[case]
    mat, rgb, params = scenes.SCENES[scene](0)
    params = dict(params, use_physical_sky=0, use_clouds=0)   # (the sky tables are test_emul_parity's)
    cfg = host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=depth, seed=3)
    return cfg, mat, rgb, params, spp


@pytest.fixture(scope="module", params=sorted(CASES))
def oracle_frames(request):
    cfg, mat, rgb, params, spp = _setup(request.param)
    o = orc.Oracle(cfg, threads=4)
    orc.setup(o, mat, rgb, params)
    o.accumulate(spp)
    frames = {"hdr": o.fetch_hdr(), **{which: o.fetch_buffer(which) for which in BUFS}}
    o.close()
    return request.param, frames


@pytest.mark.parametrize("mode", sorted(MODES))
def test_frames_are_the_oracles(lib, oracle_frames, mode):
    case, want = oracle_frames
    cfg, mat, rgb, params, spp = _setup(case)
    cap, spoil = MODES[mode]
    e = NativeSession(lib, "emu_", cfg)
    orc.setup(e, mat, rgb, params)
    counts = (C.c_ulonglong * 3)()
    assert lib.emu_accumulate_primary(C.c_void_p(e._ctx), spp, 1, cap, spoil, counts) == 0
    finished, sent_on, leftovers = (int(x) for x in counts)
    print(f"{case} {mode}: finished {finished}, sent on {sent_on}, leftovers {leftovers}")
    got = {"hdr": e.fetch_hdr(), **{which: e.fetch_buffer(which) for which in BUFS}}
    e.close()
    pixels = cfg.width * cfg.height * spp
    assert finished > 0 and sent_on > 0
    if mode == "rule":   # (three eighths of a head's items: on a frame of 64 tiles a head of eight tiles can run over, and may)
        assert finished + sent_on + leftovers == pixels
    else:
        assert sent_on <= 64 * spp and leftovers > 0 and finished + sent_on + leftovers == pixels
    for k in want:
        assert np.array_equal(want[k].view(np.uint8), got[k].view(np.uint8)), (case, mode, k)


def test_sanitized_stand_alone_program(tmp_path):
    """The host build of the stage under AddressSanitizer and UndefinedBehaviorSanitizer: pool alone, rule's queue, bounded and spoilt."""
    exe = str(tmp_path / "primary_vertex_main")
    src = os.path.join(HERE, "emul", "primary_vertex_main.cpp")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"] + HOST_FLAGS + ["-o", exe, src],
                   check=True, capture_output=True)
    for case in sorted(CASES):
        cfg, mat, rgb, params, spp = _setup(case)
        path = str(tmp_path / f"{case}.case")
        with open(path, "wb") as f:
            f.write(bytes(cfg))
            f.write(bytes(host.make_scene_params(**params)))
            f.write(bytes(host.default_camera(cfg.width, cfg.height)))
            f.write(np.uint32(1).tobytes())
            f.write(np.ascontiguousarray(mat, dtype=np.int8).tobytes())
            f.write(np.ascontiguousarray(rgb, dtype=np.uint8).tobytes())
            f.write(np.ascontiguousarray(materials.load_table(), dtype=np.float32).tobytes())
        r = subprocess.run([exe, path], capture_output=True, text=True)
        print(case, r.stdout.strip())
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
        assert r.stdout.strip().endswith("frames that differ 0")
