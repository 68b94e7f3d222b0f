"""CPU: the argument checks of tcow_attn_temporal_step_probs (csrc/attention_stream_probs.hip) against both builds of the library, and the host
checks of ops.attn_temporal_step_probs.  The entry point takes the record of tcow_attn_temporal_step and its validator: every case of
test_stream_attn_refusals_host.py must be refused here too, under THIS symbol's name, except that `out` may be NULL; probs == NULL is refused
in addition.  Every check returns before the launch and none reads through a pointer, so no GPU is needed; no case is valid: nothing launches."""
import ctypes

import pytest
import torch

from test_stream_attn_refusals_host import ATTN, ATTN_CASES, BUILDS, SOME, _id, attn_record
from tcow_amd import _lib, ops
from tcow_amd._lib import TcowError

ENTRY = 'tcow_attn_temporal_step_probs'
CASES = [c for c in ATTN_CASES if c[1] != 'out']


@pytest.mark.parametrize('fmt', BUILDS)
def test_null_args_are_refused_first(fmt):
    lib = _lib.lib(fmt)
    assert lib.tcow_attn_temporal_step_probs(None, None, SOME) == -1
    message = lib.tcow_last_error().decode()
    assert message.startswith(ENTRY + ': ') and 'args' in message, message


@pytest.mark.parametrize('fmt', BUILDS)
@pytest.mark.parametrize('form,field,value,text', CASES, ids=[_id(c) for c in CASES])
def test_each_check_of_the_record_refuses_under_this_symbol(fmt, form, field, value, text):
    lib = _lib.lib(fmt)
    status = lib.tcow_attn_temporal_step_probs(None, ctypes.byref(attn_record(form, **{field: value})), SOME)
    message = lib.tcow_last_error().decode()
    assert status == -1, (form, field, value, status, message)
    assert message.startswith(ENTRY + ': ') and text in message, (form, field, value, message)
    with pytest.raises(TcowError, match=ENTRY + ' failed'):
        _lib.check(status, ENTRY, lib)


@pytest.mark.parametrize('fmt', BUILDS)
@pytest.mark.parametrize('form', list(ATTN))
@pytest.mark.parametrize('out', [SOME, None])
def test_null_probs_is_refused_and_out_is_not_asked_for(fmt, form, out):
    """A valid record with probs == NULL: refused for probs -- also when out is NULL, which therefore is no refusal of its own."""
    lib = _lib.lib(fmt)
    status = lib.tcow_attn_temporal_step_probs(None, ctypes.byref(attn_record(form, out=out)), None)
    message = lib.tcow_last_error().decode()
    assert status == -1 and message == ENTRY + ': probs is NULL', (form, out, status, message)


def test_the_step_still_reports_under_its_own_name():
    lib = _lib.lib('bf16')
    assert lib.tcow_attn_temporal_step(None, ctypes.byref(attn_record('stream', out=None))) == -1
    assert lib.tcow_last_error().decode() == 'tcow_attn_temporal_step: null pointer'


# ---------------------------------------------------------------------------------------------- the ops wrapper

class _Lib:
    """A stand-in for a build: keeps (entry, record fields, probs pointer)."""

    def __init__(self):
        self.calls = []

    def tcow_attn_temporal_step_probs(self, stream, args, probs):
        self.calls.append((ENTRY, args._obj.out, args._obj.k_cache, probs))
        return 0


@pytest.fixture
def lib(monkeypatch):
    L = _Lib()
    monkeypatch.setattr(_lib, 'lib', lambda fmt='bf16': L)
    monkeypatch.setattr(ops, '_stream', lambda: 77)
    monkeypatch.setattr(ops, '_need_cuda', lambda *ts: None)
    return L


S, HEADS, T_TOTAL, D = 3, 2, 40, 128


def _call(form, probs, cdt=torch.float32, cache_dtype=None):
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    kc = torch.zeros(4, S - 1, HEADS, T_TOTAL, 64, dtype=cdt)
    if form == 'stream':
        return ops.attn_temporal_step_probs('stream', ops.F32, 2, 3, S, D, HEADS, 1, T_TOTAL, i32(1), torch.zeros(6 * S, 3 * D), kc, kc, probs,
                                            cache_dtype=cache_dtype), kc
    if form == 'pool':
        return ops.attn_temporal_step_probs('pool', ops.F32, 2, 3, S, D, HEADS, 1, T_TOTAL, 4, i32(2), i32(2), torch.zeros(6 * S, 3 * D), kc, kc, probs,
                                            cache_dtype=cache_dtype), kc
    tabs = (i32(3), i32(3), i32(3), i32(6))
    if form == 'ragged':
        return ops.attn_temporal_step_probs('ragged', ops.F32, 3, 6, S, D, HEADS, 1, T_TOTAL, 4, i32(3), i32(3), *tabs[1:], torch.zeros(6 * S, 3 * D), kc, kc,
                                            probs, cache_dtype=cache_dtype), kc
    return ops.attn_temporal_step_probs('paged', ops.F32, 3, 6, S, D, HEADS, 1, T_TOTAL, 17, 8, i32(3), i32(3, 5), *tabs[1:], torch.zeros(6 * S, 3 * D), kc, kc,
                                        probs, cache_dtype=cache_dtype), kc


@pytest.mark.parametrize('form', ['stream', 'pool', 'ragged', 'paged'])
def test_wrapper_passes_probs_and_leaves_out_null(lib, form):
    probs = torch.zeros(6, S - 1, HEADS, T_TOTAL)
    got, kc = _call(form, probs)
    assert got is probs and lib.calls == [(ENTRY, None, kc.data_ptr(), probs.data_ptr())]


@pytest.mark.parametrize('form', ['stream', 'pool', 'ragged', 'paged'])
def test_wrapper_refuses_a_wrong_probs_tensor(lib, form):
    n = 6 * (S - 1) * HEADS * T_TOTAL
    for bad in (torch.zeros(n - 1), torch.zeros(n + T_TOTAL), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.bfloat16),
                torch.zeros(6, S - 1, HEADS, 2 * T_TOTAL)[..., ::2], None):
        with pytest.raises(TcowError, match=rf'attn_temporal_step_probs: probs must be a contiguous float32 tensor of .* = {n} elements'):
            _call(form, bad)
    assert lib.calls == []


def test_wrapper_applies_the_host_checks_of_tables_and_cache_dtypes(lib):
    probs = torch.zeros(6, S - 1, HEADS, T_TOTAL)
    with pytest.raises(TcowError, match='attn_temporal_step_probs: cache_dtype=3 needs torch.float8_e4m3fn caches'):
        _call('ragged', probs, cache_dtype=ops.FP8)
    with pytest.raises(TcowError, match='attn_temporal_step_probs: t0_rows must be a contiguous int32 tensor of 3 entries'):
        ops.attn_temporal_step_probs('ragged', ops.F32, 3, 6, S, D, HEADS, 1, T_TOTAL, 4, torch.zeros(2, dtype=torch.int32), *[torch.zeros(3, dtype=torch.int32)] * 3,
                                     torch.zeros(6, dtype=torch.int32), torch.zeros(6 * S, 3 * D), probs, probs, probs)
    with pytest.raises(TcowError, match='attn_temporal_step_probs: qkv must have F \\* S = 18 rows'):
        ops.attn_temporal_step_probs('ragged', ops.F32, 3, 6, S, D, HEADS, 1, T_TOTAL, 4, *[torch.zeros(3, dtype=torch.int32)] * 4,
                                     torch.zeros(6, dtype=torch.int32), torch.zeros(5 * S, 3 * D), probs, probs, probs)
    with pytest.raises(TcowError, match="form='rows' must be one of"):
        ops.attn_temporal_step_probs('rows')
    assert lib.calls == []
