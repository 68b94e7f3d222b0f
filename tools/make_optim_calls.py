"""Writes tests/golden/optim_calls.json.gz: the normalised optimizer steps of every case of tests/optim_calls.py, recorded on the CPU from the
tcow_amd package that is importable (the repository's, or the one PYTHONPATH puts first -- the fixture is generated from the commit BEFORE the
optimizer's three entry points became one and must not be regenerated to make a changed trace pass).

A package of that age still calls tcow_adamw_clip_step_scaled and tcow_adamw_clip_step_cast with positional arguments: their decoders live here.

    python tools/make_optim_calls.py [output path]
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import optim_calls as kit  # noqa: E402


def old_entries(rec):
    """The two entry points of ABI <= 14 in the terms of tcow_adamw_args: without a flat table the chunk table is the flat table."""
    def scaled(build, stream, chunks, n_chunks, lr, beta1, beta2, eps, weight_decay, step, max_norm, scratch, inv_scale):
        rec.launch(build, chunks, n_chunks, chunks, n_chunks, None, 0, (lr, beta1, beta2, eps, weight_decay), step, max_norm, scratch, inv_scale)
        return 0

    def cast(build, stream, chunks, n_chunks, flat, n_flat, tiles, n_tiles, lr, beta1, beta2, eps, weight_decay, step, max_norm, scratch, inv_scale):
        rec.launch(build, chunks, n_chunks, flat, n_flat, tiles, n_tiles, (lr, beta1, beta2, eps, weight_decay), step, max_norm, scratch, inv_scale)
        return 0
    return {'tcow_adamw_clip_step_scaled': scaled, 'tcow_adamw_clip_step_cast': cast}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else kit.FIXTURE
    entries = old_entries if 'tcow_adamw_clip_step_cast' in kit._lib.SIGNATURES else kit.step_entries
    traces = {}
    for name in kit.CASES:
        with pytest.MonkeyPatch.context() as mp:
            traces[name] = kit.run_case(name, mp, entries)
        print(f'{name}: {len(traces[name])} entries')
    kit.save_fixture(traces, out)
    print(f'{out}: {os.path.getsize(out)} bytes, tcow_amd from {os.path.dirname(kit._lib.__file__)}, entry points {sorted(entries(None))}')


if __name__ == '__main__':
    main()
