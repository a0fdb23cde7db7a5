"""The launch pipeline's decisions (voxel_rt2_amd/csrc/vrt_plan.h: render kernel variant, shape, deferral depth, fused sample count,
timer period, dispatch gate, workgroups, set and lane of a launch) as plain functions, compiled for the host (tests/emul/plan_emul.cpp).  The expected
values are literals: what the library decided before the decisions were lifted out of vrt_accumulate.  No GPU."""
import ctypes as C
import itertools

import pytest

from plan import lib, shape, variant

P1080 = 1920 * 1080
DEEP = 12 << 20

# (items, heavy, queues) -> (n_streams, grid_div), defer_k (None: the issue's table states no K for the case)
SHAPES = [
    (P1080 * 4, False, 4, (2, 2), 4),      # the queue-lean shape
    (P1080 * 4, False, 6, (4, 2), 4),
    (P1080 * 4, False, 16, (4, 2), 4),
    (P1080 * 4, False, 5, (2, 2), None),   # lean
    (P1080, False, 16, (8, 4), 1),
    (P1080, False, 15, (4, 2), None),
    (P1080, False, 4, (2, 2), 4),
    (P1080, True, 16, (8, 4), None),       # heavy: 4 147 200 <= 9 * 2^19
    (2400000, True, 16, (4, 2), None),
    (DEEP, False, 16, (4, 2), None),       # exactly the deep limit
    (DEEP + 1, False, 16, (2, 1), 1),
    (3840 * 2160 * 4, False, 16, (2, 1), 1),
]


@pytest.mark.parametrize("items,heavy,queues,want,want_k", SHAPES)
def test_pipeline_shape(items, heavy, queues, want, want_k):
    assert P1080 * 4 == 8294400 and P1080 == 2073600
    got, k, pass_on_render = shape(items, queues, heavy=heavy)
    assert got == want
    assert not pass_on_render
    if want_k is not None:
        assert k == want_k
    # a context whose launches are never deferred pays for no copies, whatever the shape
    assert shape(items, queues, heavy=heavy, can_defer=False) == (want, 1, False)


def test_development_overrides():
    assert lib().plan_max_sets() == 12
    assert shape(P1080 * 4, 4, streams=3, defer4=4)[:2] == ((3, 2), 4)
    assert shape(P1080 * 4, 4, streams=2, grid_div=1, defer4=4)[:2] == ((2, 1), 1)
    assert shape(P1080 * 4, 16, pass_stream=1)[2] is True
    assert shape(P1080 * 4, 16, pass_stream=0)[2] is False
    assert shape(P1080 * 4, 16)[2] is False
    # VRT_DEFER=8: K 8 at four streams, clamped to VRT_MAX_SETS - n_streams = 12 - 8 at eight, 8 at two streams of half-size launches
    assert shape(P1080 * 4, 16, defer4=8, defer8=8)[:2] == ((4, 2), 8)
    assert shape(P1080, 16, defer4=8, defer8=8)[:2] == ((8, 4), 4)
    assert shape(P1080 * 4, 4, defer4=8, defer8=8)[:2] == ((2, 2), 8)
    assert shape(P1080 * 4, 16, streams=2, grid_div=2, defer4=8, defer8=8)[:2] == ((2, 2), 8)


def test_dispatch_gate():
    L = lib()
    # four streams of half-size launches: launch 10 takes the slots of launch 8, which raises the word to 9
    assert L.plan_target(10, 0, 2, 0, 0) == 9
    assert L.plan_wait(9, 7, 1, 1) == 1      # the lane's last launch was number 6: the wait is queued
    # two streams in steady state: the lane's last launch IS number 8 -- stream order says what the wait would
    assert L.plan_wait(9, 9, 1, 1) == 0
    assert L.plan_target(10, 1, 2, 0, 0) == 10   # the previous launch took every slot: its own drain
    assert L.plan_target(10, 1, 4, 3, 0) == 10
    assert L.plan_target(10, 0, 2, 0, 10) == 10  # never for a launch older than the last full one
    assert L.plan_target(10, 0, 4, 0, 8) == 8
    assert L.plan_target(10, 0, 4, 0, 0) == 7
    assert L.plan_target(10, 0, 2, 1, 0) == 8    # VRT_GATE_EXTRA=1
    assert L.plan_target(0, 1, 2, 0, 0) == 0 and L.plan_wait(0, 0, 1, 1) == 0   # the first launch waits for nothing
    assert L.plan_target(1, 0, 2, 0, 0) == 0
    assert L.plan_wait(9, 7, 0, 1) == 0      # no gate
    assert L.plan_wait(9, 7, 1, 0) == 0      # the most recent launch was not given the signal
    assert L.plan_wait(9, 8, 1, 1) == 1 and L.plan_wait(9, 0, 1, 1) == 1 and L.plan_wait(9, 10, 1, 1) == 0


def test_workgroups_of_a_partial_launch():
    L = lib()
    assert L.plan_blocks(512, 2) == 256
    assert L.plan_blocks(520, 2) == 264
    assert L.plan_blocks(520, 4) == 136
    assert L.plan_blocks(520, 1) == 520 and L.plan_blocks(516, 1) == 520   # whole rounds of the 8 XCDs


def test_timer_period():
    L = lib()
    assert L.plan_deep_items() == DEEP
    assert L.plan_period(0, 0, P1080 * 4) == 8
    assert L.plan_period(0, 0, DEEP) == 8
    assert L.plan_period(0, 0, DEEP + 1) == 1
    assert L.plan_period(0, 1, P1080) == 1       # ReSTIR
    assert L.plan_period(5, 0, P1080) == 5 and L.plan_period(5, 1, DEEP + 1) == 5


def test_fused_sample_count():
    L = lib()
    assert L.plan_fused(9, 1, 4) == 4
    assert L.plan_fused(1, 1, 4) == 1
    assert L.plan_fused(3, 0, 4) == 1
    assert L.plan_fused(3, 1, 4) == 3
    assert L.plan_fused(4, 1, 4) == 4 and L.plan_fused(5, 1, 2) == 2 and L.plan_fused(2, 1, 1) == 1


def test_set_and_lane_take_turns():
    L = lib()
    # two streams, K = 4: six copies; four streams, K = 4: eight
    assert [L.plan_set(q, 6) for q in range(8)] == [0, 1, 2, 3, 4, 5, 0, 1]
    assert [L.plan_lane(q, 2) for q in range(5)] == [0, 1, 0, 1, 0]
    assert (L.plan_set(13, 8), L.plan_lane(13, 4)) == (5, 1)
    assert (L.plan_set(2**32 - 1, 12), L.plan_lane(2**32 - 1, 8)) == (3, 7)


# the dense random fill: its solids reach every face of the grid (nothing to cull), half its bricks and more hold a voxel, its sun emits
DENSE_4K = dict(width=3840, height=2160, cull_active=False, dense_grid=True, light_emits=True)
# what the project runs -> the RenderVariant fields that are set (the kernel follows: vrt_plan.h)
VARIANTS = [
    ("bench config 1: S1, 256x256, 1 spp", dict(width=256, height=256, fused=1), {"pooled", "cull", "black_sun"}),                    # k_render_pool<G, 0, 1, 1>
    ("bench config 2: S1, 1080p, 4 spp", dict(), {"pooled", "cull", "black_sun", "share_primary"}),
    ("bench config 3: S6, sky + clouds + ReSTIR", dict(use_restir=True, light_emits=True), {"pooled", "restir", "cull", "share_primary"}),   # k_render_pool_restir<G, 0, 1>
    ("bench config 4: dense 128^3, 4K", DENSE_4K, {"pooled", "dense12", "share_primary"}),                                          # k_render_pool_dense12<G, 0, 0>
    ("bench config 5: dense 256^3, 4K", DENSE_4K, {"pooled", "dense12", "share_primary"}),                                          # (the grid size picks G, not the variant)
    ("sunlit, 1 spp", dict(light_emits=True, fused=1), {"pooled", "cull"}),                                                         # k_render_pool<G, 0, 0, 1>
    ("instrumented: every ray walked, no shared camera rays", dict(instrumented=True), {"pooled", "instr", "black_sun"}),
    ("instrumented, counting as the timed schedule", dict(instrumented=True, count_as_timed=True), {"pooled", "instr", "cull", "black_sun", "share_primary"}),
    ("reference indexing", dict(ref_oob=True), {"pooled", "instr", "black_sun"}),
    ("reference indexing, counting as the timed schedule", dict(ref_oob=True, instrumented=True, count_as_timed=True), {"pooled", "instr", "black_sun", "share_primary"}),
    ("VRT_RENDER=fused", dict(knob_render=0), {"cull", "black_sun"}),                                                               # k_render<G, 0, 0>
    ("VRT_RENDER=pool", dict(knob_render=1), {"pooled", "cull", "black_sun", "share_primary"}),
    ("8192 wide: 12-bit pixel coordinates do not hold it", dict(width=8192, height=1080), {"cull", "black_sun"}),
    ("4097 high", dict(height=4097), {"cull", "black_sun"}),
    ("4096 x 4096, depth 15: the largest pooled context", dict(width=4096, height=4096, max_depth=15), {"pooled", "cull", "black_sun", "share_primary"}),
    ("depth 16: 4 bits do not hold it", dict(max_depth=16), {"cull", "black_sun"}),
    ("dense on the fused schedule", dict(DENSE_4K, width=8192), set()),
    ("VRT_CULL=0", dict(knob_cull=0), {"pooled", "black_sun", "share_primary"}),
    ("VRT_CULL=1 does not force a box the scene has not", dict(knob_cull=1, cull_active=False), {"pooled", "black_sun", "share_primary"}),
    ("dense grid under a black sun: no shadow rays to speak of", dict(DENSE_4K, light_emits=False), {"pooled", "black_sun", "share_primary"}),
    ("dense grid with ReSTIR", dict(DENSE_4K, use_restir=True), {"pooled", "restir", "share_primary"}),
]


@pytest.mark.parametrize("inputs,want", [v[1:] for v in VARIANTS], ids=[v[0] for v in VARIANTS])
def test_render_variant(inputs, want):
    assert variant(**inputs) == want


def test_render_variant_every_combination():
    """plan_render_variant against its rules restated here, over every combination of the boolean inputs, at sizes on both sides of
    each limit of the pooled kernel, every value of the two switches and fused counts on both sides of 1."""
    sizes = [(64, 40, 5), (4096, 4096, 15), (4097, 40, 5), (64, 4097, 5), (64, 40, 16)]
    n = 0
    for (W, H, depth), render, cull_knob, fused in itertools.product(sizes, (-2, -1, 0, 1), (-1, 0, 1), (1, 2, 4)):
        for restir, instrumented, timed, oob, cull_active, dense, emits in itertools.product((False, True), repeat=7):
            pooled = W <= 4096 and H <= 4096 and depth <= 15 and render != 0
            instr = instrumented or oob
            want = {
                "pooled": pooled,
                "restir": restir,
                "instr": instr,
                "cull": cull_active and not (instrumented and not timed) and not oob and cull_knob != 0,
                "black_sun": not emits,
                "dense12": pooled and not restir and dense and emits,
                "share_primary": pooled and fused > 1 and (not instr or timed),
            }
            got = variant(W, H, depth, render, cull_knob, restir, instrumented, timed, oob, cull_active, dense, emits, fused)
            assert got == {k for k, on in want.items() if on}, (W, H, depth, render, cull_knob, fused, restir, instrumented, timed, oob, cull_active, dense, emits)
            n += 1
    assert n == 5 * 4 * 3 * 3 * 2 ** 7


def test_tri_layout():
    """plan_tri_layout, the one layout of the scratch vrt_voxelize_triangles and vrt_fill_triangles share: regions in order and apart, each
    as large as what it holds and aligned for what is stored there, and the buffer no more than 255 bytes larger than the two layouts
    it replaces asked for (written out here as they stood)."""
    up = lambda v: (v + 255) & ~255
    n = 0
    for head, nv, batch in itertools.product((4, 252, 256, 4 * 315), (1, 255, 256, 315, 128 ** 3), (1, 3, 1 << 18, 1 << 20)):
        out = (C.c_longlong * 5)()
        lib().plan_tri(head, nv, batch, out)
        mat_at, rgb_at, entries_at, heads_at, size = out
        key = (head, nv, batch)
        assert 0 < mat_at < rgb_at < entries_at < heads_at < size, key
        assert mat_at >= head and rgb_at - mat_at >= nv and entries_at - rgb_at >= 3 * nv and heads_at - entries_at >= 16 * batch, key
        assert entries_at % 16 == 0 and heads_at % 8 == 0 and size - heads_at >= 256, key
        assert size <= up(up(head) + up(nv) + 3 * nv) + 16 * batch + 256 + 255, key          # the fill's layout, head = 4 * words
        if head == 4 * nv:
            assert size <= up(4 * nv + up(nv) + 3 * nv) + 16 * batch + 256 + 255, key         # the surface pass's
        n += 1
    assert n == 4 * 5 * 4
