"""Shading terms the render kernels take from a table or in a shorter form -- the packed material row the pooled kernels stage,
the basis of a face normal, a texel byte over 255, the sun cone's pdf worked out with the frame's parameters -- against the
expressions they replace, on the host build of the device headers (tests/emul/shade_tables_emul.cpp).  Bit patterns, never
tolerances.  No GPU needed."""
import importlib.util
import math
import os

import numpy as np
import pytest

import emu
import shade_tables as st
from voxel_rt2_amd import materials

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def random_rows(n, seed):
    """Material rows with every parameter live, and among them the corners mat_derive() can trip on: anisotropic and
    clearcoat_gloss at 0 and at 1, metallic = 1 (diffuse weight 0), roughness 0, clearcoat 0."""
    rng = np.random.default_rng(seed)
    rows = rng.random((n, 14), dtype=np.float32)
    for col, period, value in ((8, 5, 0.0), (8, 7, 1.0), (12, 6, 0.0), (12, 11, 1.0), (4, 9, 1.0), (7, 13, 0.0), (11, 4, 0.0), (5, 17, 1.0)):
        rows[::period, col] = value
    rows[3::50, 8] = 1.0
    rows[3::50, 12] = 1.0
    rows[3::50, 4] = 1.0   # all three corners in one row
    return rows


@pytest.mark.parametrize("derive_while_staging", [False, True])
def test_packed_row_holds_the_raw_columns_and_mat_derive(derive_while_staging):
    table = materials.load_table()
    assert table.shape == (128, 14)
    for rows in (table, random_rows(4000, 21)):
        got, want = st.packed_rows(rows, derive_while_staging)
        assert np.array_equal(bits(got), bits(want)), f"{(bits(got) != bits(want)).any(axis=1).sum()} rows differ"
        # the eight raw columns are the row's own (subsurface .. roughness, sheen, sheen_tint, clearcoat)
        assert np.array_equal(bits(got[:, :8]), bits(np.ascontiguousarray(rows[:, [3, 4, 5, 6, 7, 9, 10, 11]])))


def test_face_normal_basis_equals_ortho_basis_for_every_normal_code():
    normals, got, want, fast = st.normal_bases()
    assert np.array_equal(bits(got), bits(want))
    nonzero = (normals != 0.0).sum(axis=1)
    # exactly one component of magnitude 1 -- 6 axes x 4 sign combinations of the two zeros -- takes the short form ...
    assert np.array_equal(fast == 1, nonzero == 1)
    assert int(fast.sum()) == 24
    # ... and every signed-zero combination is among them
    single = normals[fast == 1]
    assert len({tuple(bits(n).tolist()) for n in single}) == 24
    # tie normals (two or three non-zero components) and the zero normal go through the guard to ortho_basis()
    assert int((fast == 0).sum()) == 40 and set(nonzero[fast == 0].tolist()) == {0, 2, 3}


def test_byte_over_255_is_the_division_for_every_byte():
    got, want, id_got, id_want = st.bytes_over_255()
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(want, (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32))   # (the division itself, correctly rounded)
    assert np.array_equal(id_got, id_want) and np.array_equal(id_got, np.arange(256))
    enc = np.arange(256, dtype=np.uint32)
    enc = (enc << 8) | (((enc * 7 + 3) & 255) << 16) | (((255 - enc) & 255) << 24) | 2
    a, b = st.unpack_albedo(enc)
    assert np.array_equal(bits(a), bits(b))


def test_frame_constants_equal_the_device_expressions():
    cones = [0.1, 0.0, 1e-3, 0.02, 0.5, 1.0, 2.0, math.pi, 2.0 * math.pi]          # scene.py's default light_cone first
    cos_max = [np.float32(math.cos(c * 0.5)) for c in cones]
    cos_max += [np.float32(1.0) - np.float32(2.0 ** -24), np.float32(1.0), np.float32(-1.0), np.float32(0.0)]
    cos_max += list(np.cos(np.linspace(0.0, math.pi, 97)).astype(np.float32))
    cos_max = np.array(cos_max, dtype=np.float32)
    assert cos_max[9] < 1.0 and bits(cos_max[9:10])[0] == 0x3F7FFFFF
    cos_theta = np.concatenate([cos_max, np.nextafter(cos_max, np.float32(2.0)), np.nextafter(cos_max, np.float32(-2.0)),
                                np.array([1.0, -1.0, 0.0, np.nan], dtype=np.float32)])
    got, unset, want = st.cone_pdfs(cos_max, cos_theta)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(unset), bits(want))      # a parameter block whose maker left the field 0
    assert np.isinf(want[10, -4]) and want[9, -4] > 1e6  # cos_max = 1: a division by zero, as in place
    uv = [(u, v) for u in (0, 1, 2, 3, 957, 1918, 1919) for v in (0, 1, 539, 1078, 1079)]
    for W, H in ((1920, 1080), (64, 40), (3840, 2160), (50, 30)):
        a, b = st.texcoords(uv, W, H)
        assert np.array_equal(bits(a), bits(b))


def check_fixture(session, name):
    got = mg.run_case(session, mg.CASES[name])
    want = np.load(os.path.join(HERE, "golden", name + ".npz"))
    assert sorted(want.files) == sorted(got.keys())
    for key in want.files:
        assert np.array_equal(np.ascontiguousarray(got[key]).view(np.uint8), want[key].view(np.uint8)), f"{name}: {key} differs from the fixture"
    return got


@pytest.mark.parametrize("derive_while_staging", [False, True])
@pytest.mark.parametrize("name", ["s1_64x64_d4", "sunlit_80x48_d6"])
def test_pooled_emulation_with_packed_rows_equals_the_inline_path(name, derive_while_staging, monkeypatch):
    """The pooled schedule's stage functions with path_shade() reading packed rows (what the pooled kernels stage) against the
    committed fixture and against the same emulation deriving inline (emul.cpp, whose SceneData leaves the table unset)."""
    cfg = mg.config_of(mg.CASES[name])
    packed = st.PackedRows(cfg, derive_while_staging)
    got = check_fixture(packed, name)
    packed.close()
    monkeypatch.setenv("VRT_EMU_POOL", "1")
    monkeypatch.delenv("VRT_EMU_CULL", raising=False)
    inline = emu.Emulated(cfg)
    ref = mg.run_case(inline, mg.CASES[name])
    inline.close()
    for key in ref:
        assert np.array_equal(np.ascontiguousarray(got[key]).view(np.uint8), np.ascontiguousarray(ref[key]).view(np.uint8)), key
