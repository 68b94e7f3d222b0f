"""CPU: every step of FusedAdamWClip as the library sees it -- build, tables, scalars, scratch length, inverse scale, rebuilt or reused -- and the
counters it keeps, entry for entry against the fixture recorded before the optimizer's three entry points became tcow_adamw_clip_step and its
host arithmetic moved to tcow_amd/optim_plan.py (tests/optim_calls.py, tools/make_optim_calls.py)."""
import pytest

import optim_calls as kit


@pytest.fixture(scope='module')
def pinned():
    return kit.load_fixture()


def test_the_fixture_holds_exactly_the_cases(pinned):
    assert sorted(pinned) == sorted(kit.CASES)


@pytest.mark.parametrize('name', sorted(kit.CASES))
def test_steps_are_the_pinned_ones(name, pinned, monkeypatch):
    want, got = pinned[name], kit.run_case(name, monkeypatch)
    for k, (w, g) in enumerate(zip(want, got)):
        if w != g and w[0] == g[0] == 'step' and w[1]['launch'] and g[1]['launch']:
            differ = sorted(f for f in w[1]['launch'] if w[1]['launch'][f] != g[1]['launch'].get(f))
            assert not differ and w[1]['tables'] == g[1]['tables'], f"{name}: step at entry {k}: tables {w[1]['tables']} -> {g[1]['tables']}, fields that differ: {differ}"
        assert w == g, f'{name}: entry {k} of {len(want)} differs\n  expected {w}\n  actual   {g}'
    assert len(got) == len(want), f'{name}: {len(got)} entries, expected {len(want)}'


def _steps(trace):
    return [b for w, b in trace if w == 'step']


def test_the_cases_cross_what_they_are_meant_to(pinned):
    """The events the cases exist for occur in the pinned traces (a case that no longer reaches them pins nothing)."""
    tables = lambda name: [s['tables'] for s in _steps(pinned[name])]
    counters = lambda name: [b for w, b in pinned[name] if w == 'counters']
    noted = lambda name, what: [b for w, b in pinned[name] if w == what]
    assert tables('three-steps') == ['rebuilt', 'reused', 'reused']
    first = _steps(pinned['three-steps'])[0]['launch']
    assert [r[4] for r in first['chunks']] == [1, 3, 4, 7, 65536, 65536, 1, 15] and first['flat'] == first['chunks'] and first['tiles'] == []
    assert first['chunks'][5][:4] == [[5, w, 0] for w in 'pgmv'] and first['chunks'][6][:4] == [[5, w, 4 * 65536] for w in 'pgmv']
    assert tables('grad-replaced') == ['rebuilt', 'rebuilt', 'reused', 'rebuilt'] and [c['skipped_steps'] for c in counters('grad-replaced')] == [0.0, 1.0, 1.0, 2.0]
    assert tables('grad-none') == ['rebuilt', 'rebuilt', 'reused', None]
    assert tables('load-state-dict') == ['rebuilt', 'reused', 'rebuilt', 'reused'] and noted('load-state-dict', 'saved steps') == [[1.0] * 7]
    assert [s['launch']['step'] for s in _steps(pinned['load-state-dict'])] == [1, 2, 2, 3]          # the loaded count is the applied one
    assert [s['launch']['step'] for s in _steps(pinned['late-gradient'])] == [1, 2, 3, 4, 5]         # the base is the maximum, whoever comes first
    assert counters('late-gradient')[2]['steps'][4] == 1.0 and counters('late-gradient')[3]['steps'][0] == 1.0
    assert noted('state-dict-with-skips', 'saved steps') == [[1.0] * 7] and noted('state-dict-with-skips', 'live steps') == [[3.0] * 7 + [None]]
    assert [('one parameter group' in r, 'contiguous f32' in r) for r in noted('refusals', 'refused')] == [(True, False), (False, True), (False, True)]
    for p, build in (('bf16', 'bf16'), ('fp16', 'fp16'), ('fp32', 'bf16')):
        fuse, nofuse = _steps(pinned[f'module-{p}-fuse']), _steps(pinned[f'module-{p}-nofuse'])
        assert [s['tables'] for s in fuse] == ['rebuilt', 'reused', 'reused', 'rebuilt', 'rebuilt', 'rebuilt', 'reused']      # the generation moved three times
        assert [s['tables'] for s in nofuse][:5] == ['rebuilt', 'reused', 'reused', 'reused', 'reused']                          # and nobody looked
        assert all(not s['launch']['tiles'] and s['launch']['build'] == 'bf16' for s in nofuse)
        tiles = [len(s['launch']['tiles']) for s in fuse]
        assert tiles == ([73, 73, 73, 0, 73, 73, 73] if p != 'fp32' else [0] * 7) and all(len(s['launch']['chunks']) == 69 for s in fuse)
        assert [s['launch']['build'] for s in fuse] == [build if t else 'bf16' for t in tiles]
        assert all(s['launch']['inv_scale'] == (p == 'fp16') for s in fuse)
    assert [s['launch']['inv_scale'] for s in _steps(pinned['fp16-scale'])] == [True, False, True, True, True, True]
    assert [c['ls_log2'] for c in counters('fp16-scale')] == [-2.0, -2.0, -6.0, -6.0 + 1 / 256, -6.0 + 2 / 256, -6.0 + 2 / 256]
    assert noted('unscale-detach-fp16', 'pending_inv_scale') == [True, False] and noted('unscale-detach-bf16', 'pending_inv_scale') == [False, False]
    assert noted('unscale-detach-fp16', 'after unscale_') == [[True, True]] and noted('unscale-detach-fp16', 'after detach') == [[True, True]]
