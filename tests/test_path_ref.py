"""tests/path_ref.c through its six views (tests/emission_ref.py to tests/lamp_ref.py), without a GPU: every case of
tests/golden/path_ref_pins.json — recorded from the six separate references those views replaced, by
tests/golden/make_path_ref_pins.py at the commit before them — comes out bit for bit: the frames' hashes, the counts, the load
planes and arrivals, the lens rays and the traced pixels.  And the pins are worth holding to: no counter is zero in all of them."""
import json

import pytest

from golden import make_path_ref_pins as P

PINS = P.load_pins()


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    return P.Context(tmp_path_factory.mktemp("path_ref"))


@pytest.mark.parametrize("view", list(P.VIEWS))
def test_the_view_gives_what_its_own_reference_gave(ctx, view):
    want = {name: case for name, case in PINS.items() if name.split("/")[0] == view}
    got = P.record(ctx, view)
    assert list(got) == list(want)
    for name, case in got.items():
        assert json.dumps(case) == json.dumps(want[name]), name   # (as text: the sign of a zero counts)


def test_every_case_belongs_to_a_view():
    assert {name.split("/")[0] for name in PINS} == set(P.VIEWS)


def test_no_counter_is_zero_in_every_case():
    assert P.never_zero(PINS) == []
    assert P.never_zero({name: case for name, case in PINS.items() if not name.startswith("lamp/44x28")}) == ["load_lamp", "load_path", "load_sun"]
