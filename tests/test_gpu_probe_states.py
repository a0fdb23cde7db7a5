"""vrt_gather_probes ON THE DEVICE on contexts in every frame state, bit for bit against the oracle on a context that has no such
state: the query promises to read scene data only (include/vrt_api.h), so its answer must not notice ReSTIR, a moving camera, a render
scale below 1, frames in flight, a pending deferred accumulation, a row tile, row stripes, a reset, instrumented launches or reserved
CUs.  tests/states.py holds the states (imported, not edited); tests/probe.py the expected values and the comparison: floats by their
bits, no row left out.
  - every state x its cases: the probes at 3 samples on the device path, `query` being vrt_trace_radiance on that same stated context;
  - all at once: `everything` (ReSTIR, reserved CUs, instrumented, a moving camera at a render scale, frames queued and not waited
    for) is one of the states; and the interleaving with frames -- gathers queued after each of three launches whose deferred pass
    is pending -- compared with the oracle's records once the context is waited for."""
import pytest

import probe as P
import states as T
from voxel_rt2_amd import _abi, _lib
from voxel_rt2_amd._session import NativeSession

pytestmark = pytest.mark.gpu

SAMPLES = T.SENSOR_SAMPLES


def device_gather(s, probes, samples, first_frame=P.FIRST_FRAME, sync=True):
    return T._device(s, lambda i, o: s.gather_probes(i, samples, first_frame, o), probes, _abi.SH_PROBE, sync)


def check_probes(s, case, label):
    probes = P.probes_of(case)
    want = P.expected(case, SAMPLES, T.device_query(s))
    P.check(device_gather(s, probes, SAMPLES), probes, want, f"{label}: probes x {SAMPLES} samples, device path")


@pytest.mark.parametrize("state,case", T.PAIRS)
def test_probes_do_not_notice_the_frame_state(state, case):
    s = T.open_session(P, case, state)
    try:
        with T.stats_unchanged(s, state == "instrumented"):
            check_probes(s, case, f"{state}/{case}")
        if state in T.AFTER:
            T.AFTER[state](s)
    finally:
        s.close()


def test_results_of_gathers_interleaved_with_frames_equal_the_oracle():
    """accumulate(4) x 3 at 64 x 40 under the overlapped pipeline, a device-path gather queued after every call and kept; every one
    finds a deferred accumulation pending (tests/states.py: deferral())."""
    case = "sunlit_d5"
    assert T.deferral() > 3
    probes = P.probes_of(case)
    s = P.start(NativeSession(_lib.load(), "vrt_", P.config(case, 64, 40)), case)
    try:
        kept = []
        for k in range(3):
            s.accumulate(4)
            kept.append(device_gather(s, probes, SAMPLES, sync=False))
        want = P.expected(case, SAMPLES, T.device_query(s))                             # (host-path queries: they force no pass either)
        s.sync()
        for k, got in enumerate(kept):
            P.check(T.read_back(got, _abi.SH_PROBE), probes, want, f"probes queued after launch {k}")
        T.AFTER["big_frame"](s)
    finally:
        s.close()
