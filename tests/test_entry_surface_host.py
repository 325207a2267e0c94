"""The host surface of the sampler entry points against tests/golden/g23_entry_errors.json: signatures and docstrings of
the 16 Plan methods, every _lib.SYMBOLS entry, and -- no device is needed for it -- the refusal of a null plan by each of
the 18 C entry points."""
import inspect

import pytest

from eeyore_amd import _lib as L
from tests import entry_error_cases as E

REC = E.load_record()


@pytest.mark.parametrize("method", E.PLAN_METHODS)
def test_plan_method_signature_and_docstring(method):
    from eeyore_amd.plan import Plan
    fn = getattr(Plan, method)
    assert str(inspect.signature(fn)) == REC["signatures"][method]
    assert fn.__doc__ == REC["docs"][method]


def test_symbols_are_the_recorded_ones():
    assert {name: E.symbol_text(entry) for name, entry in L.SYMBOLS.items()} == REC["symbols"]


@pytest.mark.parametrize("entry", E.ENTRIES)
def test_null_plan_is_refused_with_the_recorded_text(entry):
    rc, msg = E.null_plan_call(entry)
    want = [REC["cases"][E.record_key("c", entry, w, "null_plan")] for w in ("f32", "f64")]
    assert rc != 0 and all((rc, msg) == (r["status"], r["message"]) for r in want)
