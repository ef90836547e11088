"""CPU: the brightest pixel, the average Y and the colour statistics of the back end's edge pictures (tests/backend_images.py) as the compiled
reference computed them (tests/golden/backend_reductions.json, written by tests/golden/make_backend_reductions.py): exact ties everywhere
in flat fields, the raster tie-break against decode order, the unsigned luminance sum past 2^32, saturated colour fields.  The oracle must
reproduce every record -- the GPU tests (tests/test_gpu_backend_tiling.py) check the HIP path against the oracle, so this pins what they
check to the reference itself -- and so must the compiled reference where it is built."""
import json
import os

import pytest

import backend_images as BI

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backend_reductions.json")


@pytest.fixture(scope="module")
def cases(harness):
    return BI.golden_cases(harness)


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_pictures_are_the_recorded_ones(harness, cases, want):
    assert sorted(cases) == sorted(want)
    for name, data in cases.items():
        assert harness.hash_bytes(data) == want[name]["sha256"], name


def test_the_records_pin_the_edges(want):
    """What the records must show for the tests built on them to mean anything."""
    for name, r in want.items():
        if name.startswith("flat_"):
            y = {"white": 1017, "black": -1023, "grey": 0}[name.rsplit("_", 1)[1]]
            assert r["bright_avg"][1] == y and r["bright_avg"][7:9] == [0, 0], name    # every pixel ties: the first one, MCU (0,0)
    for layout in ("420", "440"):
        assert want["raster_tie_" + layout]["bright_avg"][7:9] == [9, 0]                # the raster order, not the decode order
    w, h = BI.WRAP_SIZE
    for layout in ("420", "gray"):
        avg = want["wrap_%s_white" % layout]["bright_avg"][9]
        assert avg == (w * h * 255 % 2 ** 32) // ((w + 1) * (h + 1)) and avg < 255      # the sum wrapped: far below 255


def test_oracle_and_reference_reproduce_the_records(harness, cases, want):
    backends = [harness.oracle_backend()] + ([harness.ref_backend()] if harness.have_ref() else [])
    try:
        for b in backends:
            for name, data in sorted(cases.items()):
                assert BI.record(harness, b, data) == want[name], (b.name, name)
    finally:
        for b in backends:
            b.close()
