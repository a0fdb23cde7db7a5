"""The oracle's row bands (host.make_config(..., rows=)) equal the same rows of its whole frame, under every call pattern that
tests/test_gpu_bench_frames.py compares the GPU's frames with bands under: repeated fused calls, then one-sample calls with a
new jitter and end_frame; on S1, dense 128^3 and dense 256^3, the dense grids in both indexing modes.  CPU only."""
import functools

import numpy as np
import pytest

import bands
from voxel_rt2_amd import host, scenes

W, H, DEPTH, SEED = 160, 96, 8, 3
SNAPSHOTS = [3, 8]                    # after the fused calls, and at the end
ROWS = [(0, 8), (43, 52), (88, 96)]   # top, a band off the 8x8 wave-tile grid, bottom


@functools.lru_cache(maxsize=None)
def scene(name):
    return scenes.SCENES[name](12345 if name.startswith("dense") else 0)


def calls():
    """Three fused calls of 4 samples on the set-up camera (jitter 1), then five frames of the Scene API's loop: jitters 2..6,
    one sample, end_frame."""
    return [4, 4, 4] + [(1, host.default_camera(W, H, jitter_index=k)) for k in range(2, 7)]


@pytest.mark.parametrize("name,grid", [("s1", 128), ("dense", 128), ("dense256", 256)])
def test_oracle_bands_equal_full_frames(name, grid):
    modes = (False, True) if name.startswith("dense") else (False,)
    full = {}
    for ref in modes:
        kw = dict(depth=DEPTH, seed=SEED, grid=grid, ref_indexing=ref, threads=8)
        frames = bands.oracle_band(scene(name), W, H, (0, H), calls(), SNAPSHOTS, **kw)
        full[ref] = frames[SNAPSHOTS[-1]][0]
        assert np.isfinite(full[ref]).all() and full[ref].mean() > 0.01
        assert bands.first_difference(frames[SNAPSHOTS[0]][0], full[ref]) is not None   # the one-sample frames changed the image
        for rows in ROWS:
            part = bands.oracle_band(scene(name), W, H, rows, calls(), SNAPSHOTS, **kw)
            for k in SNAPSHOTS:
                bands.assert_rows_equal(part[k][0], frames[k][0][rows[0]:rows[1]], rows[0],
                                        f"{name}, reference indexing {ref}, rows {rows} after {k} calls")
    if len(modes) == 2:
        # the bands hold pixels where the two indexing modes differ: the reference-mode comparison above has teeth
        differ = sum(int((full[False][a:b] != full[True][a:b]).any(-1).sum()) for a, b in ROWS)
        assert differ > 0, "no pixel of the bands differs between the indexing modes"
