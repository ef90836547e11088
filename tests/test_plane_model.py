"""CPU: tests/plane_model.py, the numpy model the GPU tests of jsnoop_batch_pack_planes compare against, pinned on its own -- the U8 formula over every
int16, NATIVE against the replication the oracle's decode left in its planes (4:2:0, 4:2:2, 4:4:0, 4:1:1), NATIVE luma against FULL luma, and the size
arithmetic at the smallest dimensions."""
import numpy as np
import pytest

from plane_model import expand_factors, fma_telling_values, one_rounding, plane_dims, plane_model, two_roundings, u8_value

LAYOUTS = {"4:2:0": (2, 2), "4:2:2": (2, 1), "4:4:0": (1, 2), "4:1:1": (4, 1)}


def test_u8_is_the_clamped_shift_for_every_int16():
    """min(max((v + 1024) / 8, 0), 255) with truncating division == clip((v >> 3) + 128, 0, 255): the two differ only where the numerator is -7 .. -1,
    below the clamp."""
    v = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
    shift = np.clip((v.astype(np.int64) >> 3) + 128, 0, 255).astype(np.uint8)
    assert np.array_equal(u8_value(v), shift)
    n = v.astype(np.int64) + 1024
    c_div = np.array([int(x / 8) if x >= 0 else -int(-x / 8) for x in range(-40, 41)])            # C's n / 8 next to zero, spelled out
    assert np.array_equal(np.where(n >= 0, n // 8, -((-n) // 8))[(n >= -40) & (n <= 40)], c_div)
    assert (u8_value(np.int16(-1025)), u8_value(np.int16(-1024)), u8_value(np.int16(-1017)), u8_value(np.int16(-1016))) == (0, 0, 0, 1)
    assert (u8_value(np.int16(1015)), u8_value(np.int16(1016)), u8_value(np.int16(32767)), u8_value(np.int16(-32768))) == (254, 255, 255, 0)
    m = plane_model(v.reshape(256, 256), 256, 256, 1, 1, "full", "uint8")
    assert m.dtype == np.uint8 and np.array_equal(m.ravel(), shift)


@pytest.fixture(scope="module")
def oracle_planes(harness, oracle):
    out = {}
    for k, (name, (hs, vs)) in enumerate(LAYOUTS.items()):
        for w, h in ((45, 37), (64, 32)):
            f = harness.synth_jpeg(width=w, height=h, hs=hs, vs=vs, quality=90, seed=900 + k)
            harness.drive(oracle, f)
            ps = [p.copy() for p in oracle.planes()]
            assert all(p is not None and p.shape[0] >= h and p.shape[1] >= w for p in ps)
            out[(name, w, h)] = ps
    return out


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_native_then_repeat_gives_the_replicated_plane_back(oracle_planes, name):
    hs, vs = LAYOUTS[name]
    for (nm, w, h), ps in oracle_planes.items():
        if nm != name:
            continue
        for c, (eh, ev) in enumerate(expand_factors(hs, vs)):
            nat = plane_model(ps[c], w, h, eh, ev, "native")
            assert nat.shape == (-(-h // ev), -(-w // eh)) and nat.dtype == np.int16
            back = np.repeat(np.repeat(nat, ev, axis=0), eh, axis=1)[:h, :w]
            assert np.array_equal(back, ps[c][:h, :w]), (name, w, h, c)
            assert np.array_equal(plane_model(ps[c], w, h, eh, ev, "full"), ps[c][:h, :w])
        assert len({int(x) for x in ps[1][:h, :w].ravel()}) > 4, "a chroma plane with content"


def test_native_luma_equals_full_luma(oracle_planes):
    for (nm, w, h), ps in oracle_planes.items():
        for dtype in ("int16", "uint8", "float32"):
            assert np.array_equal(plane_model(ps[0], w, h, 1, 1, "native", dtype, 0.1, 0.3), plane_model(ps[0], w, h, 1, 1, "full", dtype, 0.1, 0.3))


@pytest.mark.parametrize("eh,ev", [(1, 1), (2, 2), (2, 1), (1, 2), (4, 1), (3, 4)])
def test_size_arithmetic_at_the_smallest_dimensions(eh, ev):
    P = (np.arange(64 * 64, dtype=np.int32).reshape(64, 64) - 2000).astype(np.int16)
    for dx, wx in ((1, 1), (eh, 1), (eh + 1, 2)):
        for dy, wy in ((1, 1), (ev, 1), (ev + 1, 2)):
            assert plane_dims(dx, dy, eh, ev, "native") == (wy, wx) and plane_dims(dx, dy, eh, ev, "full") == (dy, dx)
            m = plane_model(P, dx, dy, eh, ev, "native")
            assert m.shape == (wy, wx) and m[0, 0] == P[0, 0] and m[-1, -1] == P[(wy - 1) * ev, (wx - 1) * eh]
            assert plane_model(P, dx, dy, eh, ev, "full").shape == (dy, dx)


def test_float_form_is_two_roundings_and_the_constants_tell_a_fused_one_apart():
    scale, bias = (0.1, 1 / 3, 0.7), (0.3, -1 / 7, 1e-3)
    tell = fma_telling_values(scale, bias)
    assert all(len(t) > 0 for t in tell)
    for c in range(3):
        v = np.array(tell[c], np.int16).reshape(1, -1)
        m = plane_model(v, v.shape[1], 1, 1, 1, "full", "float32", scale[c], bias[c])
        assert m.dtype == np.float32
        for j, x in enumerate(tell[c]):
            assert float(m[0, j]) == two_roundings(x, scale[c], bias[c]) != one_rounding(x, scale[c], bias[c])
