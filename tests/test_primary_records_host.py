"""primary_record_walk() (csrc/vrt_pool.h) -- what k_primary_records stores ahead of a launch -- gives, for every pixel and word for
word, the record the pooled schedule leaves for sample 0: BEGIN's set-up and, where there is something to walk, the WALK stage over
the slot's packed fields (tests/emul/primary_emul.cpp steps both on the host build of the device headers).  No GPU.

Frames of 48 x 40 on s1, sunlit, dense and s1_256 from three poses of tests/poses.py -- the default one, one inside the grid and one
looking away from it (every camera ray culled) -- with the scene's culling box and with the open one, whole frames and a row tile
whose first row is no multiple of 8.  The same frames go through a stand-alone program built with -fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import poses
import primary

W, H = 48, 40
SCENES = ("s1", "sunlit", "dense", "s1_256")
POSES = ("default", "in_grid", "away")
TAG = 0x1234


def _config(name, rows=None):
    cfg = poses.config(name, W, H)
    if rows:
        cfg.row_begin, cfg.row_end = rows
    return cfg


def _session(name, rows=None):
    mat, rgb, params = poses.scene(name)
    s = primary.Session(_config(name, rows))
    poses.start(s, name)
    return s


@pytest.fixture(scope="module", params=SCENES)
def session(request):
    s = _session(request.param)
    yield request.param, s
    s.close()


@pytest.mark.parametrize("cull", [True, False], ids=["cull", "open_box"])
@pytest.mark.parametrize("pose", POSES)
def test_walk_record_is_the_schedules_record(session, pose, cull):
    name, s = session
    s.set_camera(poses.cam(W, H, pose, jitter_index=POSES.index(pose)))
    by_walk, by_schedule, walked = s.records(cull, TAG)
    same = (by_walk == by_schedule).all(-1)
    print(f"{name} {pose} cull={cull}: {int(walked.sum())} of {walked.size} camera rays walked")
    assert same.all(), f"{int((~same).sum())} records differ, first (v, u) {np.argwhere(~same)[:4].tolist()}"
    # the records are this launch's and nobody else's, and not the zeros the arrays started as
    assert all(primary.record_valid(by_walk[v, u], TAG) and not primary.record_valid(by_walk[v, u], TAG + 1) for v, u in ((0, 0), (H // 2, W // 2), (H - 1, W - 1)))
    assert by_walk[..., 3:6].any(-1).all(), "every record carries a direction"
    if pose == "away" and cull and name != "dense":   # (the dense scene fills the grid: its box is the grid, and the camera is in it)
        assert not walked.any(), "looking away from the scene's box, nothing is walked"
    if pose == "default":
        assert walked.any()


def test_the_frames_are_not_trivial():
    """Walked rays that end on a voxel, on nothing, and rays that are never walked all occur on s1's default pose."""
    s = _session("s1")
    s.set_camera(poses.cam(W, H, "default"))
    rec, _, walked = s.records(True, TAG)
    s.close()
    t = rec[..., 0].view(np.float32)
    assert (walked & np.isfinite(t)).any() and (walked & np.isinf(t)).any() and (~walked).any()
    assert len(np.unique(rec[walked][:, 1])) > 20, "many different cells"


def test_row_tile_with_an_odd_first_row():
    """Rows 13..31 (the context buffers 11..33): the records of a row tile are the frame's records of those rows."""
    whole, tile = _session("sunlit"), _session("sunlit", rows=(13, 31))
    for s in (whole, tile):
        s.set_camera(poses.cam(W, H, "default", jitter_index=5))
    a, a_sched, _ = whole.records(True, TAG)
    b, b_sched, _ = tile.records(True, TAG)
    r0, r1 = tile.buffered_rows()
    whole.close(); tile.close()
    assert (r0, r1) == (11, 33) and b.shape[0] == r1 - r0
    assert np.array_equal(b, b_sched) and np.array_equal(a[r0:r1], b)


def test_the_jitter_moves_the_records():
    """Another jitter index is another camera ray: a record made for one launch must not pass for another's (the tag's job)."""
    s = _session("s1")
    s.set_camera(poses.cam(W, H, "default", jitter_index=0))
    a = s.records(True, TAG)[0]
    s.set_camera(poses.cam(W, H, "default", jitter_index=1))
    b = s.records(True, TAG)[0]
    s.close()
    assert not np.array_equal(a[..., 3:6], b[..., 3:6])


def test_sanitized_stand_alone_program(tmp_path):
    """The host build of primary_record_walk() under AddressSanitizer and UndefinedBehaviorSanitizer, over the same frames."""
    exe = str(tmp_path / "primary_records_main")
    src = os.path.join(primary.HERE, "emul", "primary_records_main.cpp")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"] + primary.HOST_FLAGS + ["-o", exe, src],
                   check=True, capture_output=True)
    for name in SCENES:
        mat, rgb, params = poses.scene(name)
        from voxel_rt2_amd import host
        case = str(tmp_path / f"{name}.case")
        cams = [poses.cam(W, H, pose, jitter_index=k) for k, pose in enumerate(POSES)]
        with open(case, "wb") as f:
            f.write(bytes(_config(name)))
            f.write(bytes(host.make_scene_params(**params)))
            f.write(np.uint32(len(cams)).tobytes())
            for cam in cams:
                f.write(bytes(cam))
            f.write(np.ascontiguousarray(mat, dtype=np.int8).tobytes())
            f.write(np.ascontiguousarray(rgb, dtype=np.uint8).tobytes())
        r = subprocess.run([exe, case], capture_output=True, text=True)
        print(name, r.stdout.strip())
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
        assert f"frames {2 * len(POSES)} records {2 * len(POSES) * W * H} " in r.stdout and r.stdout.strip().endswith("mismatches 0")
