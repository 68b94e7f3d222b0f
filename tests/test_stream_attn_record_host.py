"""CPU: the record each of the seven stream wrappers of tcow_amd.ops hands to the library (tcow_stream_attn_args / tcow_stream_cls_args), field by field
against expectations written out by hand.  The library is a stand-in that keeps what it is given (one per build); ops._stream and ops._need_cuda are
replaced as in tests/engine_trace.py, so the wrappers take CPU tensors and every pointer field can be compared with the tensor it must name."""
import ctypes

import pytest
import torch

from tcow_amd import _lib, ops
from tcow_amd._lib import TcowError

S, D, HEADS, T_TOTAL = 3, 128, 2, 40
F32, BF16, FP8 = _lib.TCOW_F32, _lib.TCOW_BF16, _lib.TCOW_FP8E4M3
# (mode, cache_dtype keyword) -> (build that is called, shape.dtype, cache_dtype of the record, torch dtype of qkv / out, of the caches).
# None fills in the storage type; F32X3 stores as F32; the FP16 mode goes to the binary16 build with ABI dtype TCOW_BF16.
EXPECT = {(ops.F32, None): ('bf16', F32, F32, torch.float32, torch.float32), (ops.F32, ops.BF16): ('bf16', F32, BF16, torch.float32, torch.bfloat16),
          (ops.F32, ops.FP8): ('bf16', F32, FP8, torch.float32, torch.float8_e4m3fn),
          (ops.BF16, None): ('bf16', BF16, BF16, torch.bfloat16, torch.bfloat16), (ops.BF16, ops.BF16): ('bf16', BF16, BF16, torch.bfloat16, torch.bfloat16),
          (ops.BF16, ops.FP8): ('bf16', BF16, FP8, torch.bfloat16, torch.float8_e4m3fn),
          (ops.FP16, None): ('fp16', BF16, BF16, torch.float16, torch.float16), (ops.FP16, ops.BF16): ('fp16', BF16, BF16, torch.float16, torch.float16),
          (ops.FP16, ops.FP8): ('fp16', BF16, FP8, torch.float16, torch.float8_e4m3fn),
          (ops.F32X3, None): ('bf16', F32, F32, torch.float32, torch.float32), (ops.F32X3, ops.BF16): ('bf16', F32, BF16, torch.float32, torch.bfloat16),
          (ops.F32X3, ops.FP8): ('bf16', F32, FP8, torch.float32, torch.float8_e4m3fn)}


def _fields(rec):
    out = {}
    for name, _ in rec._fields_:
        v = getattr(rec, name)
        out[name] = _fields(v) if isinstance(v, ctypes.Structure) else v
    return out


class Build:
    """One build of the library: the two step entry points keep (build, entry, stream, record fields) and return `status`."""

    def __init__(self, name, calls):
        self.name, self.calls, self.status = name, calls, 0

    def _entry(self, entry):
        def call(stream, args):
            assert isinstance(args._obj, {'tcow_attn_temporal_step': _lib.StreamAttnArgs, 'tcow_cls_step': _lib.StreamClsArgs}[entry])
            self.calls.append((self.name, entry, stream, _fields(args._obj)))
            return self.status
        return call

    def __getattr__(self, name):
        if name in ('tcow_attn_temporal_step', 'tcow_cls_step'):
            return self._entry(name)
        raise AttributeError(name)                                  # (none of the former entry points, nothing else)

    def tcow_last_error(self):
        return b'the message of the library'


@pytest.fixture
def calls(monkeypatch):
    got = []
    builds = {b: Build(b, got) for b in ('bf16', 'fp16')}
    monkeypatch.setattr(_lib, 'lib', lambda fmt='bf16': builds[fmt])
    monkeypatch.setattr(ops, '_stream', lambda: 77)
    monkeypatch.setattr(ops, '_need_cuda', lambda *ts: None)
    return got, builds


def _i32(*shape):
    return torch.zeros(*shape, dtype=torch.int32)


def _p(t):
    return None if t is None else t.data_ptr()


ATTN_REST = dict(n_sessions=0, n_slots=0, page_frames=0, n_pages=0, pages_per_session=0, slot_rows=None, first_rows=None, c_rows=None, row_of_frame=None,
                 page_rows=None)


def _attn_case(form, mode, cq):
    """(the wrapper call, the record it must make) of one form under one (mode, cache_dtype keyword)."""
    _, dm, cache_dtype, dt, cdt = EXPECT[mode, cq]
    rows = 6                                                        # 2 rows x 3 frames, or 6 flat frames of sessions of 3, 1, 2
    qkv, out = torch.zeros(rows * S, 3 * D, dtype=dt), torch.zeros(rows * S, D, dtype=dt)
    cache = lambda *lead: (torch.zeros(*lead, S - 1, HEADS, 4, 64).to(cdt), torch.zeros(*lead, S - 1, HEADS, 4, 64).to(cdt))
    t0, slot, first, c, rof, pages = _i32(2), _i32(2), _i32(3), _i32(3), _i32(6), _i32(3, 5)
    t0_1, t0_3, slot_3 = _i32(1), _i32(3), _i32(3)
    shape_rows = dict(B=2, T=3, S=S, D=D, heads=HEADS, causal=2, dtype=dm)
    shape_flat = dict(B=1, T=6, S=S, D=D, heads=HEADS, causal=2, dtype=dm)
    if form == 'cached':
        k, v = cache(2)
        call = lambda: ops.attn_temporal_cached(mode, 2, 3, S, D, HEADS, 2, T_TOTAL, t0_1, qkv, k, v, out, cache_dtype=cq)
        want = dict(ATTN_REST, shape=shape_rows, t0_rows=_p(t0_1))                                  # the stream: no slot table, n_slots left to the library
    elif form == 'pool':
        k, v = cache(5)
        call = lambda: ops.attn_temporal_pool(mode, 2, 3, S, D, HEADS, 2, T_TOTAL, 5, t0, slot, qkv, k, v, out, cache_dtype=cq)
        want = dict(ATTN_REST, shape=shape_rows, n_slots=5, t0_rows=_p(t0), slot_rows=_p(slot))
    elif form == 'ragged':
        k, v = cache(5)
        call = lambda: ops.attn_temporal_ragged(mode, 3, 6, S, D, HEADS, 2, T_TOTAL, 5, t0_3, slot_3, first, c, rof, qkv, k, v, out, cache_dtype=cq)
        want = dict(ATTN_REST, shape=shape_flat, n_sessions=3, n_slots=5, t0_rows=_p(t0_3), slot_rows=_p(slot_3), first_rows=_p(first), c_rows=_p(c),
                    row_of_frame=_p(rof))
    else:
        k, v = cache(17)
        call = lambda: ops.attn_temporal_ragged_paged(mode, 3, 6, S, D, HEADS, 2, T_TOTAL, 17, 8, t0_3, pages, first, c, rof, qkv, k, v, out, cache_dtype=cq)
        want = dict(ATTN_REST, shape=shape_flat, n_sessions=3, page_frames=8, n_pages=17, pages_per_session=5, t0_rows=_p(t0_3), first_rows=_p(first),
                    c_rows=_p(c), row_of_frame=_p(rof), page_rows=_p(pages))                        # pages, not slots: no slot table, n_slots 0
    want.update(cache_dtype=cache_dtype, T_total=T_TOTAL, qkv=_p(qkv), k_cache=_p(k), v_cache=_p(v), out=_p(out))
    return call, want, out


@pytest.mark.parametrize('form', ['cached', 'pool', 'ragged', 'ragged_paged'])
@pytest.mark.parametrize('mode,cq', list(EXPECT), ids=[f'{m}-{c}' for m, c in EXPECT])
def test_attention_wrapper_fills_the_record(calls, form, mode, cq):
    got, _ = calls
    call, want, out = _attn_case(form, mode, cq)
    assert call() is out
    assert got == [(EXPECT[mode, cq][0], 'tcow_attn_temporal_step', 77, want)]
    assert sorted(want) == sorted(f for f, _ in _lib.StreamAttnArgs._fields_)                      # every field of the record is expected above


def test_cls_wrappers_fill_the_record(calls):
    got, _ = calls
    x, cache = torch.zeros(6 * S, D), torch.zeros(5, D)
    t0_1, t0, slot, t0_3, slot_3, first, c = _i32(1), _i32(2), _i32(2), _i32(3), _i32(3), _i32(3), _i32(3)
    assert ops.cls_stream(x, 2, 3, S, cache, t0_1) is x
    assert ops.cls_pool(x, 2, 3, S, cache, 5, t0, slot) is x
    assert ops.cls_ragged(x, 3, 6, S, cache, 5, t0_3, slot_3, first, c) is x
    base = dict(S=S, D=D, x=_p(x), cls_cache=_p(cache), first_rows=None, c_rows=None)
    assert got == [('bf16', 'tcow_cls_step', 77, dict(base, n=2, c=3, F=0, n_slots=0, t0_rows=_p(t0_1), slot_rows=None)),     # the stream: no slot table
                   ('bf16', 'tcow_cls_step', 77, dict(base, n=2, c=3, F=0, n_slots=5, t0_rows=_p(t0), slot_rows=_p(slot))),
                   ('bf16', 'tcow_cls_step', 77, dict(base, n=3, c=0, F=6, n_slots=5, t0_rows=_p(t0_3), slot_rows=_p(slot_3), first_rows=_p(first), c_rows=_p(c)))]
    assert all(sorted(rec) == sorted(f for f, _ in _lib.StreamClsArgs._fields_) for _, _, _, rec in got)


def test_errors_carry_the_symbol_and_the_wrappers_own_checks_their_name(calls):
    got, builds = calls
    call, _, _ = _attn_case('pool', ops.FP16, ops.FP8)
    builds['fp16'].status = -1
    with pytest.raises(TcowError, match=r'tcow_attn_temporal_step failed \(status -1\): the message of the library'):
        call()
    builds['bf16'].status = -1
    with pytest.raises(TcowError, match=r'tcow_cls_step failed \(status -1\)'):
        ops.cls_pool(torch.zeros(6 * S, D), 2, 3, S, torch.zeros(5, D), 5, _i32(2), _i32(2))
    del got[:]
    # the torch-dtype check of the caches runs for a keyword that is not None, under the wrapper's name, before any call; None checks nothing
    qkv, out, k16 = torch.zeros(6 * S, 3 * D), torch.zeros(6 * S, D), torch.zeros(2, S - 1, HEADS, 4, 64, dtype=torch.bfloat16)
    for who, run in (('attn_temporal_cached', lambda cd, k: ops.attn_temporal_cached(ops.F32, 2, 3, S, D, HEADS, 1, T_TOTAL, _i32(1), qkv, k, k, out, cache_dtype=cd)),
                     ('attn_temporal_pool', lambda cd, k: ops.attn_temporal_pool(ops.F32, 2, 3, S, D, HEADS, 1, T_TOTAL, 2, _i32(2), _i32(2), qkv, k, k, out, cache_dtype=cd)),
                     ('attn_temporal_ragged', lambda cd, k: ops.attn_temporal_ragged(ops.F32, 3, 6, S, D, HEADS, 1, T_TOTAL, 2, _i32(3), _i32(3), _i32(3), _i32(3), _i32(6),
                                                                                     qkv, k, k, out, cache_dtype=cd)),
                     ('attn_temporal_ragged_paged', lambda cd, k: ops.attn_temporal_ragged_paged(ops.F32, 3, 6, S, D, HEADS, 1, T_TOTAL, 2, 8, _i32(3), _i32(3, 5), _i32(3),
                                                                                                 _i32(3), _i32(6), qkv, k, k, out, cache_dtype=cd))):
        for cd, needs in ((ops.FP8, 'torch.float8_e4m3fn'), (ops.F32, 'torch.float32')):
            with pytest.raises(TcowError, match=f'^{who}: cache_dtype={cd} needs {needs} caches, got torch.bfloat16 / torch.bfloat16'):
                run(cd, k16)
        assert got == []
    # 0 page frames / 0 sessions would select another form of the record: the wrappers refuse them, in the library's words for the neighbouring values
    empty = _i32(0)
    with pytest.raises(TcowError, match=r'^attn_temporal_ragged_paged: page_frames=0 must be a power of two'):
        ops.attn_temporal_ragged_paged(ops.F32, 3, 6, S, D, HEADS, 1, T_TOTAL, 2, 0, _i32(3), _i32(3, 5), _i32(3), _i32(3), _i32(6), qkv, k16, k16, out)
    with pytest.raises(TcowError, match=r'^attn_temporal_ragged: a ragged step is one row of F frames of 1 <= n <= F sessions \(F=6 n=0\)'):
        ops.attn_temporal_ragged(ops.F32, 0, 6, S, D, HEADS, 1, T_TOTAL, 2, empty, empty, empty, empty, _i32(6), qkv, k16, k16, out)
    with pytest.raises(TcowError, match=r'^cls_ragged: a ragged step is one row of F frames'):
        ops.cls_ragged(torch.zeros(6 * S, D), 0, 6, S, torch.zeros(5, D), 5, empty, empty, empty, empty)
    assert got == []
    builds['bf16'].status = 0
    ops.attn_temporal_cached(ops.F32, 2, 3, S, D, HEADS, 1, T_TOTAL, _i32(1), qkv, k16, k16, out)        # None: the caches' torch dtype is not looked at
    ops.attn_temporal_cached(ops.F32, 2, 3, S, D, HEADS, 1, T_TOTAL, _i32(1), qkv, k16, k16, out, cache_dtype=9)     # unknown: passed on for the library to refuse
    assert [(c[3]['cache_dtype'], c[3]['shape']['dtype']) for c in got] == [(F32, F32), (9, F32)]
