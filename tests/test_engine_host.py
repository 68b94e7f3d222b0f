"""CPU: the launch schedule of engine.run_forward / run_backward, call for call, against the fixture recorded before the engine was split
(tests/engine_trace.py, tools/make_engine_trace.py)."""
import pytest

import engine_trace as kit


@pytest.fixture(scope='module')
def pinned():
    return kit.load_fixture()


def test_the_fixture_holds_exactly_the_cases(pinned):
    assert sorted(pinned) == sorted(kit.CASES)


@pytest.mark.parametrize('name', sorted(kit.CASES))
def test_schedule_is_the_pinned_one(name, pinned, monkeypatch):
    want, got = pinned[name], kit.run_case(name, monkeypatch)
    for k, (w, g) in enumerate(zip(want, got)):
        assert w == g, f'{name}: call {k} of {len(want)} differs\n  expected {w}\n  actual   {g}'
    assert len(got) == len(want), (f'{name}: {len(got)} calls, expected {len(want)}; first call beyond the shorter trace: '
                                   f'{(want + got)[min(len(want), len(got))]}')


def test_pointers_are_decided_by_declared_type(monkeypatch):
    """A small integer in a c_void_p position is a pointer, a large one in a c_long position is a scalar."""
    trace = kit.install(monkeypatch)
    from tcow_amd import _lib
    _lib.lib().tcow_scale_cast(0, 1, 1 << 40, 7, 5, 3, None, 9, 2)
    assert trace.calls == [['tcow_scale_cast', None, 1, 1 << 40, 7, 'ptr', 3, None, 'ptr', 2]]
    assert trace.events == [('call', 'tcow_scale_cast', [5, 9])]
