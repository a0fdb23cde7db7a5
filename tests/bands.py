"""Row bands of the CPU oracle, for comparing whole frames that only a GPU can render in reasonable time.

Every pixel has its own random stream, so a band of rows (host.make_config(..., rows=)) is the same rows of the whole frame
(tests/test_oracle_bands.py pins that for every call pattern used here).  A band always spans the whole frame width: the last
column and the 12-bit u of the pooled kernel are in every comparison."""
import numpy as np

import orc
from voxel_rt2_amd import host


def play(sess, calls):
    """Successive calls: an int n is accumulate(n); a pair (n, camera) is set_camera(camera), accumulate(n), end_frame() -- the
    Scene API's loop shape (scene.py's samples_per_frame = 1: a new jitter every frame)."""
    for c in calls:
        if isinstance(c, tuple):
            sess.set_camera(c[1])
            sess.accumulate(c[0])
            sess.end_frame()
        else:
            sess.accumulate(c)


def oracle_band(scene, W, H, rows, calls, snapshots, *, depth, seed, grid=128, ref_indexing=False, bufs=(), bufs_at=None, threads=16):
    """Rows [rows[0], rows[1]) of the oracle's frame after calls[:k] (see play) for every k in `snapshots` (a sorted list of
    call counts; len(calls) == snapshots[-1]).  The session is set up as bench.py's setup_session does: default camera, jitter index 1.
    Returns {k: (hdr rows, {buffer id: buffer rows})}, the buffers `bufs` at snapshot `bufs_at` only (None: at every one)."""
    mat, rgb, params = scene
    cfg = host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=depth, seed=seed,
                           grid_res=grid, rows=rows)
    o = orc.Oracle(cfg, threads=threads)
    try:
        orc.setup(o, mat, rgb, params, cam=host.default_camera(W, H, jitter_index=1))
        if ref_indexing:
            o.set_reference_indexing(True)
        assert len(calls) == snapshots[-1]
        out, done = {}, 0
        for k in snapshots:
            play(o, calls[done:k])
            done = k
            want = bufs if bufs_at in (None, k) else ()
            out[k] = (o.fetch_hdr()[rows[0]:rows[1]].copy(), {b: o.fetch_buffer(b)[rows[0]:rows[1]].copy() for b in want})
        return out
    finally:
        o.close()


def first_difference(got, want):
    """None if the arrays are equal bit for bit, else (number of differing pixels, (row, column) of the first one)."""
    a = np.ascontiguousarray(got).view(np.uint8).reshape(got.shape[0], got.shape[1], -1)
    b = np.ascontiguousarray(want).view(np.uint8).reshape(want.shape[0], want.shape[1], -1)
    assert a.shape == b.shape, (got.shape, want.shape)
    bad = np.argwhere((a != b).any(-1))
    if len(bad) == 0:
        return None
    return len(bad), tuple(int(i) for i in bad[0])


def assert_rows_equal(got, want, r0, what):
    """got, want: the same rows (from frame row r0) of two frames or buffers; equal bit for bit, else the first differing pixel."""
    d = first_difference(got, want)
    if d is not None:
        n, (y, x) = d
        raise AssertionError(f"{what}: {n} of {got.shape[0] * got.shape[1]} pixels differ; the first at row {r0 + y}, column {x}: "
                             f"{got[y, x]} != {want[y, x]} (expected)")


def assert_rows_differ(got, want, what):
    """Negative control: the comparison above would have noticed this difference."""
    assert first_difference(got, want) is not None, f"{what}: the rows are equal, so the comparison has no teeth here"
