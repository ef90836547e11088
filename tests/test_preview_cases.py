"""CPU: the preview model (tests/preview_model.py) against the oracle on every case of tests/preview_cases.py, and the census that
shows each case does what its name says -- a picture or a state that loses its point fails here, not silently on the GPU.

The progressive picture goes through the oracle as the baseline file of the same coefficients (the oracle refuses SOF2), so its cases
are in the census too; on the GPU its truth is the model on the decoder's own planes."""
import numpy as np
import pytest

import preview_cases as PC
import preview_model as PM

_REF = {}


def reference(H, oracle, name):
    """(picture, planes, {state: (oracle DIB, oracle bright_avg)}) of every state of the layout, set after the decode; computed once."""
    if name not in _REF:
        pic = PC.picture(H, name)
        PC.oracle_drive(H, oracle, pic)
        planes, out = PM.planes_of(oracle), {}
        try:
            for st in [PM.DEFAULT] + PC.cases_of(name):
                oracle.set_preview_mode(st[0])
                oracle.set_preview_ycc_offset(*st[1:])
                out[st] = (oracle.dib(), oracle.bright_avg())
        finally:
            oracle.set_preview_ycc_offset(0, 0, 0, 0, 0)
            oracle.set_preview_mode(1)
        _REF[name] = (pic, planes, out)
    return _REF[name]


def test_crossing_and_seam_starts():
    PC.assert_crossing()
    st = PC.starts()
    assert st["at_nmcu"][1] * PC.XMAX + st["at_nmcu"][0] == PC.XMAX * PC.YMAX and st["x_past_the_row"][0] >= PC.XMAX
    assert PC.wgs_of(PC.XMAX * PC.YMAX, PC.SEAM_MPW) == 4 and PC.wgs_of(PC.XMAX * PC.YMAX, 1) == 10          # several workgroups at both settings


@pytest.mark.parametrize("name", list(PC.LAYOUTS))
def test_model_equals_the_oracle(harness, oracle, name):
    """DIB and the ten bright_avg ints (the model's Y sum is in the last) of every state."""
    pic, planes, ref = reference(harness, oracle, name)
    assert planes[0].shape == (pic.ymax * pic.mcu_h, pic.xmax * pic.mcu_w)
    for st, (dib, ba) in ref.items():
        got, sum_y = PM.expect(oracle, planes, pic.mcu_w, pic.mcu_h, st, with_sum=True)
        assert np.array_equal(got, dib), (name, st, int((got != dib).sum()))
        assert PM.bright_avg(oracle, planes, pic.mcu_w, pic.mcu_h, sum_y) == ba, (name, st)


@pytest.mark.parametrize("name", list(PC.LAYOUTS))
def test_state_set_before_the_decode_equals_state_set_after(harness, oracle, name):
    pic, _planes, ref = reference(harness, oracle, name)
    try:
        for st in PC.cases_of(name):
            oracle.set_preview_mode(st[0])
            oracle.set_preview_ycc_offset(*st[1:])
            PC.oracle_drive(harness, oracle, pic)
            assert np.array_equal(oracle.dib(), ref[st][0]) and oracle.bright_avg() == ref[st][1], (name, st)
    finally:
        oracle.set_preview_ycc_offset(0, 0, 0, 0, 0)
        oracle.set_preview_mode(1)
    PC.oracle_drive(harness, oracle, pic)
    assert np.array_equal(oracle.dib(), ref[PM.DEFAULT][0])


@pytest.mark.parametrize("name", list(PC.LAYOUTS))
def test_census(harness, oracle, name):
    pic, planes, ref = reference(harness, oracle, name)
    H8, W8 = planes[0].shape
    for mode in PC.MODES[1:]:
        same = np.array_equal(ref[(mode, 0, 0, 0, 0, 0)][0], ref[PM.DEFAULT][0])
        assert same == PC.shows_rgb(name, mode), (name, mode, "the mode shows what mode 1 shows" if same else "grey: R, B and Y must be one value")
    for st in PC.cases_of(name):
        shift = st[3:]
        if not any(shift):
            continue
        dib = ref[st][0][::-1, :, :3]                                            # top-down
        plain = ref[(st[0], 0, 0, 0, 0, 0)][0][::-1, :, :3]
        sel = PM.shifted_mask((H8, W8), pic.mcu_w, pic.mcu_h, st[1], st[2])
        changed = (dib != plain).any(-1)
        assert not changed[~sel].any(), (name, st, "a pixel in front of the start changed")
        if not PC.inside(st):
            assert not sel.any() and not changed.any(), (name, st)
            continue
        assert sel.any()
        if PC.start_index(st) > 0:
            assert not sel[:pic.mcu_h, :pic.mcu_w].any() and np.array_equal(dib[:pic.mcu_h, :pic.mcu_w], plain[:pic.mcu_h, :pic.mcu_w])
        if shift in PC.LARGE:
            ycc = PM.shifted_samples(planes, pic.mcu_w, pic.mcu_h, st)
            beyond = [int((np.abs(ycc[..., c][sel]) > 32767).sum()) for c in range(3) if shift[c]]
            assert sum(beyond) > 0, (name, st, "no sample + shift leaves the int16 range")
        if PC.inert(name, st):
            assert not changed.any(), (name, st, "a shift of a component the mode does not show changed a pixel")
            continue
        assert changed.any(), (name, st, "the shift changes no pixel")
        # the start MCU itself, where the shift is at least one output step in a component the mode shows (the garbage of the partial
        # layouts sits at the clamps over whole MCUs, where a small shift shows nothing: not asked of them)
        if name not in PC.PARTIAL and any(abs(shift[c]) >= 8 for c in PC.VISIBLE[st[0]]):
            i = PC.start_index(st)
            y0, x0 = i // pic.xmax * pic.mcu_h, i % pic.xmax * pic.mcu_w
            assert sel[y0, x0] and (i == 0 or not sel[(i - 1) // pic.xmax * pic.mcu_h, (i - 1) % pic.xmax * pic.mcu_w])
            assert changed[y0:y0 + pic.mcu_h, x0:x0 + pic.mcu_w].any(), (name, st, "the start MCU itself does not change")
        if shift == (0, 7, 0):
            assert (~changed[sel]).any(), (name, st, "a shift below one output step changed every pixel")
