"""Every refused call of tests/entry_error_cases.py answers what tests/golden/g23_entry_errors.json recorded (status and
text of the C entry point, exception type and text of the Plan method), and leaves theta, target, grad and the sampler's
state with the bytes they had."""
import pytest

from tests import entry_error_cases as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return E.load_record()["cases"]


_worlds = {}


def _world(name):
    if name not in _worlds:
        _worlds[name] = E.World(name, "cuda:0")
    return _worlds[name]


@pytest.fixture(params=E.WORLDS)
def world(request):
    return _world(request.param)


@pytest.fixture(params=("f32", "f64"))  # Plan's own checks do not depend on the model: the refused one has C cases only
def small_world(request):
    return _world(request.param)


def test_the_record_holds_exactly_the_cases_of_the_table(recorded):
    keys = {E.record_key("c", e, w, c.name) for e in E.ENTRIES for c in E.c_cases(e) for w in c.worlds}
    keys |= {E.record_key("plan", e, w, c.name) for e, _, _ in E.plan_entries() for c in E.plan_cases(e) for w in c.worlds}
    assert keys == set(recorded)


@pytest.mark.parametrize("entry", E.ENTRIES)
def test_c_entry_point_answers_as_recorded(world, recorded, entry):
    ran = 0
    for case in E.c_cases(entry):
        if world.name in case.worlds:
            rc, msg = E.run_c(world, entry, case)
            want = recorded[E.record_key("c", entry, world.name, case.name)]
            assert (rc, msg) == (want["status"], want["message"]), (entry, case.name)
            ran += 1
    assert ran and world.changed() == []


@pytest.mark.parametrize("entry,method,base", E.plan_entries(), ids=[e for e, _, _ in E.plan_entries()])
def test_plan_method_raises_as_recorded(small_world, recorded, entry, method, base):
    world = small_world
    for case in E.plan_cases(entry):
        exc, text = E.run_plan(world, method, base, case)
        want = recorded[E.record_key("plan", entry, world.name, case.name)]
        assert (exc, text) == (want["exception"], want["text"]), (entry, case.name)
    assert world.changed() == []
