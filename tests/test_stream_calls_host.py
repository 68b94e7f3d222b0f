"""CPU: the host side of stream, pool and rollover-pool calls, entry for entry, against the fixture recorded before the host arithmetic of
tcow_amd/stream.py moved to tcow_amd/stream_plan.py (tests/stream_calls.py, tools/make_stream_calls.py)."""
import pytest

import stream_calls as kit


@pytest.fixture(scope='module')
def pinned():
    return kit.load_fixture()


def test_the_fixture_holds_exactly_the_cases(pinned):
    assert sorted(pinned) == sorted(kit.CASES)


@pytest.mark.parametrize('name', sorted(kit.CASES))
def test_calls_are_the_pinned_ones(name, pinned, monkeypatch):
    want, got = pinned[name], kit.run_case(name, monkeypatch)
    for k, (w, g) in enumerate(zip(want, got)):
        assert w == g, f'{name}: entry {k} of {len(want)} differs\n  expected {w}\n  actual   {g}'
    assert len(got) == len(want), (f'{name}: {len(got)} entries, expected {len(want)}; first entry beyond the shorter trace: '
                                   f'{(want + got)[min(len(want), len(got))]}')


@pytest.mark.parametrize('name', sorted(kit.CASES))
def test_a_refused_call_moves_nothing(name, pinned):
    """The state noted after a refused call is the state noted before it, and nothing was launched in between."""
    trace, state = pinned[name], None
    for k, (what, body) in enumerate(trace):
        if what == 'state':
            before, state = state, body
            refused = isinstance(trace[k - 1][1], dict) and 'refused' in trace[k - 1][1]
            if refused and before is not None and trace[k - 1][0] not in ('close', 'reset', 'open'):
                assert body == before and trace[k - 2][0] == 'state', (name, k, trace[k - 1])


def test_the_cases_cross_what_they_are_meant_to(pinned):
    """Per family, the events the cases exist for occur in the pinned traces (a schedule that no longer reaches them pins nothing)."""
    def refusals(name):
        return [b['refused'] for w, b in pinned[name] if isinstance(b, dict) and 'refused' in b]

    def forwards(name):
        return [b for w, b in pinned[name] if w == 'forward']
    assert any('run past the last frame' in r for r in refusals('stream'))
    for text in ('sessions given', 'is not open', 'duplicate', 'run past', 'lengths must agree', 'rgb must be', 'slots are taken', 'has no pages'):
        assert any(text in r for r in refusals('pool')), text
    assert {f['form'] for f in forwards('pool')} == {'_PoolStep'} and {f['form'] for f in forwards('ragged')} == {'_RaggedStep'}
    assert {f['cache'][1] for f in forwards('cache-fp8')} == {'torch.float8_e4m3fn'} and {f['cache'][1] for f in forwards('cache-bf16')} == {'torch.bfloat16'}
    strip = lambda t: [[w, {k: v for k, v in b.items() if k != 'cache'}] if w == 'forward' else [w, b] for w, b in t]
    assert strip(pinned['cache-fp8']) == strip(pinned['cache-bf16']) == strip(pinned['stream'])          # the keyword reaches the state and nothing else
    for name in pinned:
        if name.startswith('paged') or (name.startswith('rollover') and 'contiguous' not in name):
            assert any('out of pages' in r for r in refusals(name)), name
            assert {f['form'] for f in forwards(name)} == {'_PagedRaggedStep'}
        if name.startswith('rollover'):
            assert sum('no hand-off yet' in r for r in refusals(name)) == 2 and any('a chunk of' in r for r in refusals(name))
            states = [b for w, b in pinned[name] if w == 'state']
            assert any(s['retained'] for s in states) and max(max(s['window'].values(), default=0) for s in states) >= 2
            calls = [k for k, (w, b) in enumerate(pinned[name]) if w in ('step', 'step_ragged')]
            launches = [sum(1 for w, b in pinned[name][lo:hi] if w == 'forward') for lo, hi in zip([0] + calls, calls)]
            assert set(launches) == {0, 1, 2}                   # refused, one part, two parts
            assert sum(w == 'requery' for w, b in pinned[name]) >= 4
