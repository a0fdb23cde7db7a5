"""The camera-ray records of a launch on the host build of the device headers (tests/emul/primary_emul.cpp = emul.cpp plus
emu_primary_records): primary_record_walk() of csrc/vrt_pool.h, which k_primary_records runs ahead of a launch, beside the record
the emulated pooled schedule leaves for sample 0.  Test infrastructure of tests/test_primary_records_host.py; the sessions are
emu.Emulated's, on this library."""
import ctypes as C
import os
import subprocess

import numpy as np

from voxel_rt2_amd._session import NativeSession

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_primary_emul.so")
HOST_FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wno-unknown-pragmas"]   # (emu.build's)
_lib = None


def deps():
    csrc, inc = os.path.join(ROOT, "voxel_rt2_amd", "csrc"), os.path.join(ROOT, "include")
    return ([os.path.join(HERE, "emul", f) for f in ("primary_emul.cpp", "emul.cpp", "primary_records_main.cpp")] +
            [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")] + [os.path.join(inc, f) for f in os.listdir(inc)])


def stale(product):
    return not os.path.exists(product) or any(os.path.getmtime(d) > os.path.getmtime(product) for d in deps())


def build(force=False):
    if force or stale(_SO):
        subprocess.run(["g++", "-O2", "-fPIC", "-shared"] + HOST_FLAGS + ["-o", _SO, os.path.join(HERE, "emul", "primary_emul.cpp")],
                       check=True, capture_output=True)
    return _SO


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_SO)
        _lib.emu_primary_records.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.emu_primary_record_valid.argtypes = [C.c_void_p, C.c_uint32]
    return _lib


class Session(NativeSession):
    def __init__(self, cfg):
        super().__init__(lib(), "emu_", cfg)

    def records(self, cull, tag):
        """(by_walk, by_schedule, walked): uint32[rows, W, 8] twice and bool[rows, W], rows = the buffered rows of the context."""
        r0, r1 = self.buffered_rows()
        a, b = (np.zeros((r1 - r0, self.W, 8), dtype=np.uint32) for _ in range(2))
        walked = np.zeros((r1 - r0, self.W), dtype=np.uint8)
        rc = self._lib.emu_primary_records(C.c_void_p(self._ctx), int(cull), tag, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                                           walked.ctypes.data_as(C.c_void_p))
        assert rc == 0
        return a, b, walked.astype(bool)

    def buffered_rows(self):
        """The rows a context holds: its own and a halo of two (emu_create; ReSTIR is not used here)."""
        o0, o1 = self.rows
        return max(o0 - 2, 0), min(o1 + 2, self.H)


def record_valid(rec, tag):
    rec = np.ascontiguousarray(rec, dtype=np.uint32)
    return bool(lib().emu_primary_record_valid(rec.ctypes.data_as(C.c_void_p), tag))
