"""CPU: the argument checks of tcow_adamw_clip_step (csrc/optim.hip), against both builds of the library.  Every check returns before any launch, so
no GPU is needed; each must give a non-zero status and a message that names the entry point and the offending field."""
import ctypes

import pytest

BUILDS = ('bf16', 'fp16')
SOME = 0x1000                                   # a non-null address: no check reads through it


def _args(**kw):
    from tcow_amd import _lib
    good = dict(chunks=SOME, n_chunks=1, flat_chunks=SOME, n_flat=1, tiles=None, n_tiles=0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01,
                step=1, max_norm=0.3, scratch=SOME, grad_inv_scale=None)
    good.update(kw)
    return _lib.AdamwArgs(**good)


CASES = [('null chunks', dict(chunks=None), 'chunks'),
         ('null scratch', dict(scratch=None), 'scratch'),
         ('n_chunks < 1', dict(n_chunks=0), 'n_chunks'),
         ('n_chunks negative', dict(n_chunks=-3), 'n_chunks'),
         ('step < 1', dict(step=0), 'step'),
         ('negative flat count', dict(n_flat=-1), 'n_flat'),
         ('negative tile count', dict(n_tiles=-1), 'n_tiles'),
         ('flat count without a table', dict(flat_chunks=None, n_flat=2), 'flat_chunks'),
         ('tile count without a table', dict(tiles=None, n_tiles=5), 'tiles')]


@pytest.mark.parametrize('fmt', BUILDS)
def test_null_args_are_refused(fmt):
    from tcow_amd import _lib
    lib = _lib.lib(fmt)
    assert lib.tcow_adamw_clip_step(None, None) == -1                   # TCOW_ERR_INVALID_ARG
    message = lib.tcow_last_error().decode()
    assert 'tcow_adamw_clip_step' in message and 'args' in message


@pytest.mark.parametrize('fmt', BUILDS)
@pytest.mark.parametrize('what,change,field', CASES, ids=[c[0] for c in CASES])
def test_each_check_names_the_entry_point_and_the_field(fmt, what, change, field):
    from tcow_amd import _lib
    lib = _lib.lib(fmt)
    status = lib.tcow_adamw_clip_step(None, ctypes.byref(_args(**change)))
    message = lib.tcow_last_error().decode()
    assert status == -1, (what, status)                                 # refused by a check, never by a failed launch
    assert message.startswith('tcow_adamw_clip_step: ') and field in message.split(': ', 1)[1].split()[0], (what, message)
    with pytest.raises(_lib.TcowError, match='tcow_adamw_clip_step failed .*' + field):
        _lib.check(status, 'tcow_adamw_clip_step', lib)


def test_the_cases_differ_from_valid_arguments_in_one_field_only():
    """(what the valid set is: every case above changes it in the named place, so the message can only come from that check)"""
    good = _args()
    assert good.chunks and good.scratch and good.n_chunks >= 1 and good.step >= 1 and good.n_flat >= 0 and good.n_tiles >= 0 and good.flat_chunks and not good.tiles
    assert ctypes.sizeof(good) == 88                                    # 2 x (pointer, int, padding), pointer, int + 5 floats, int, float + 2 pointers
