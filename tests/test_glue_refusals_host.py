"""CPU: the argument checks of the glue and loss-head entry points (csrc/tokens.hip, clip_input.hip, mask_head.hip, casts.hip, mask_loss.hip,
metrics.hip, query_masks.hip, snitch_weights.hip) and their four size functions, replayed against both builds of the library.

tests/golden/glue_refusals.json was recorded by tools/make_glue_refusals.py from the commit BEFORE these sources were split by family; every
status and message must still be the recorded one, character for character.  No case reaches a launch, so no GPU is needed."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'glue_refusals.json')
BUILDS = ('bf16', 'fp16')


def call(lib, entry, args):
    """Calls lib.<entry>(*args) with the JSON form of the arguments: numbers and nulls as they are, {'mask_loss_args': [...]} = an array of
    tcow_mask_loss_args records given as field dicts.  Returns (value, tcow_last_error())."""
    from tcow_amd import _lib
    keep, argv = [], []
    for a in args:
        if isinstance(a, dict):
            jobs = a['mask_loss_args']
            arr = (_lib.MaskLossArgs * max(len(jobs), 1))(*[_lib.MaskLossArgs(**j) for j in jobs])
            keep.append(arr)
            a = ctypes.cast(arr, ctypes.POINTER(_lib.MaskLossArgs)) if jobs else None
        argv.append(a)
    value = getattr(lib, entry)(*argv)
    return value, lib.tcow_last_error().decode()


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize('fmt', BUILDS)
def test_refusals_are_the_recorded_ones(fmt):
    from tcow_amd import _lib
    lib = _lib.lib(fmt)
    cases = _fixture()['refusals'][fmt]
    assert len(cases) >= 50
    for c in cases:
        status, message = call(lib, c['entry'], c['args'])
        assert (status, message) == (c['status'], c['message']), (c['entry'], c['args'])
        assert status == -1                                            # TCOW_ERR_INVALID_ARG: refused by a check, never by a failed launch


@pytest.mark.parametrize('fmt', BUILDS)
def test_size_functions_return_the_recorded_values(fmt):
    from tcow_amd import _lib
    lib = _lib.lib(fmt)
    rows = _fixture()['sizes'][fmt]
    assert {r['entry'] for r in rows} == {'tcow_mask_loss_workspace_bytes', 'tcow_mask_loss_workspace_bytes_for', 'tcow_snitch_weights_workspace_bytes',
                                          'tcow_cast_desc_bytes'}
    for r in rows:
        assert getattr(lib, r['entry'])(*r['args']) == r['value'], (r['entry'], r['args'])
