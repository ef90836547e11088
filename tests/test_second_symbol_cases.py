"""CPU: every file of tests/second_symbol_cases.py holds the event it is named after (proved from the writer's census); the oracle decodes
the well-formed ones without raising its error state and the others with it."""
import pytest

import second_symbol_cases as SC


@pytest.mark.parametrize("i", range(len(SC.CASES)), ids=[fn.__name__ for fn in SC.CASES])
def test_case_holds_its_event(harness, oracle, i):
    c = SC.build_all()[i]
    c.check(c)
    assert c.stream.frame.width <= 128 and c.stream.frame.height <= 128 and len(c.file) < 64 * 1024
    harness.drive(oracle, c.file)
    st = oracle.status()
    if c.wellformed:
        assert not st["scan_bad"], st
        assert harness.oracle_coefs(oracle).shape[0] == len(c.stream.coefs)
    else:
        if c.group == "cut_interval":             # the reference's decode ends in the block of the cut pair, with the first symbol's value read and nothing else
            got = harness.oracle_coefs(oracle); row = got[SC.last_block_read(got)]
            assert st["scan_bad"] and row[1] == 16 and not row[2:].any(), (st, row.tolist())
        assert st["scan_bad"] or st["warn_bad"] or c.group == "cut_interval", st


def test_colour_forms_hold_their_events_too():
    cases = SC.build_all(colour=True)
    assert len(cases) >= 15
    for c in cases:
        c.check(c)
        assert c.stream.frame.ncomp == 3 and c.stream.frame.width <= 128 and c.stream.frame.height <= 128
