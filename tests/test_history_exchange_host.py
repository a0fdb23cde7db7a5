"""parallel.exchange_history on CPU: gloo process groups of 2 and 3 ranks, each with a stand-in session that serves a byte
pattern of its own for its rows and records what it is asked to import.  Every rank must import exactly every other rank's
row range, with that rank's bytes, and nothing into its own rows."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 24, 37


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def pattern(rank, row0, row1):
    """What rank `rank` exports for rows [row0, row1): the record's bytes as a function of rank, plane, row and column."""
    rec = np.empty(40 * W * (row1 - row0), dtype=np.uint8)
    n = W * (row1 - row0)
    k = 0
    for plane, size in enumerate((16, 16, 4, 4)):
        rows = np.arange(row0, row1).repeat(W * size)
        rec[k:k + n * size] = (rank * 61 + plane * 17 + rows * 5 + np.arange(n * size)) % 251
        k += n * size
    return rec


class FakeSession:
    io_on_device = False   # host memory: the recorded calls read and write it directly

    class cfg:
        device = 0

    def __init__(self, rank, rows):
        self.rank, self.rows, self.W, self.H = rank, rows, W, H
        self.exports, self.imports = [], []

    def history_rows_io(self, row0, row1, ptr, to_library):
        n = 40 * W * (row1 - row0)
        if to_library:
            self.imports.append((row0, row1, bytes((C.c_char * n).from_address(int(ptr)))))
        else:
            assert (row0, row1) == self.rows
            self.exports.append((row0, row1))
            rec = pattern(self.rank, row0, row1)   # (held while memmove reads it: a temporary would be freed before)
            C.memmove(int(ptr), rec.ctypes.data, n)

    def sync(self):
        pass


def _worker(rank, world, port, bounds, out_dir):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from voxel_rt2_amd import parallel
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    if bounds is None:
        want = parallel.split_rows(H, world)
    else:
        want = bounds
    s = FakeSession(rank, want[rank])
    parallel.exchange_history(s, rank, world, "cpu", bounds=bounds)
    got = {f"{a}_{b}": np.frombuffer(data, dtype=np.uint8) for a, b, data in s.imports}
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), exports=np.array(s.exports), order=np.array([(a, b) for a, b, _ in s.imports]), **got)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,bounds", [(2, None), (3, None), (3, [(0, 5), (5, 30), (30, 37)]), (2, [(0, 36), (36, 37)])])
def test_every_rank_imports_every_peer_range(tmp_path, world, bounds):
    from voxel_rt2_amd import parallel
    mp.spawn(_worker, args=(world, _free_port(), bounds, str(tmp_path)), nprocs=world, join=True)
    ranges = bounds if bounds is not None else parallel.split_rows(H, world)
    for rank in range(world):
        z = np.load(tmp_path / f"rank{rank}.npz")
        assert [tuple(e) for e in z["exports"]] == [ranges[rank]]
        imported = sorted(tuple(e) for e in z["order"])
        assert imported == sorted(r for q, r in enumerate(ranges) if q != rank)
        own = set(range(*ranges[rank]))
        for q, (a, b) in enumerate(ranges):
            if q == rank:
                continue
            assert not own & set(range(a, b))
            assert np.array_equal(z[f"{a}_{b}"], pattern(q, a, b)), (rank, q)
