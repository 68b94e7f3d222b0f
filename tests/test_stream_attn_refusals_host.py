"""CPU: the argument checks of tcow_attn_temporal_step and tcow_cls_step (csrc/attention_stream.hip), against both builds of the library.  Every check
returns before the launch and none reads through a pointer, so no GPU is needed: each case differs from a valid record of its form in ONE field and
must give TCOW_ERR_INVALID_ARG and a message that starts with the entry point and carries the text of that check.  No case is valid: nothing launches."""
import ctypes

import pytest

from tcow_amd import _lib

BUILDS = ('bf16', 'fp16')
SOME = 0x1000                                   # a non-null address: no check reads through it
F32, BF16, F32X3, FP8 = _lib.TCOW_F32, _lib.TCOW_BF16, _lib.TCOW_F32X3, _lib.TCOW_FP8E4M3
TENSORS = dict(qkv=SOME, k_cache=SOME, v_cache=SOME, out=SOME)
ROWS = {'shape.B': 2, 'shape.T': 3, 'shape.S': 3, 'shape.D': 128, 'shape.heads': 2, 'shape.causal': 1, 'shape.dtype': F32, 'cache_dtype': F32, 'T_total': 40}
RAGGED = dict(ROWS, **{'shape.B': 1, 'shape.T': 6, 'n_sessions': 3, 't0_rows': SOME, 'first_rows': SOME, 'c_rows': SOME, 'row_of_frame': SOME}, **TENSORS)
# the four served forms of the attention step (fields not named are 0 / NULL)
ATTN = {'stream': dict(ROWS, t0_rows=SOME, **TENSORS),
        'pool': dict(ROWS, n_slots=3, t0_rows=SOME, slot_rows=SOME, **TENSORS),
        'ragged': dict(RAGGED, n_slots=4, slot_rows=SOME),
        'paged': dict(RAGGED, page_frames=8, n_pages=17, pages_per_session=5, page_rows=SOME)}
CLS = {'stream': dict(n=2, c=3, S=3, D=128, x=SOME, cls_cache=SOME, t0_rows=SOME),
       'pool': dict(n=2, c=3, S=3, D=128, n_slots=3, x=SOME, cls_cache=SOME, t0_rows=SOME, slot_rows=SOME),
       'ragged': dict(n=3, F=6, S=3, D=128, n_slots=4, x=SOME, cls_cache=SOME, t0_rows=SOME, slot_rows=SOME, first_rows=SOME, c_rows=SOME)}


def attn_record(form, **change):
    f = dict(ATTN[form], **change)
    shape = _lib.AttnShape(**{k[6:]: f.pop(k) for k in list(f) if k.startswith('shape.')})
    return _lib.StreamAttnArgs(shape=shape, **f)


def cls_record(form, **change):
    return _lib.StreamClsArgs(**dict(CLS[form], **change))


def fields(rec):
    """{field: value} of a record as the library reads it, the shape's fields as 'shape.X'."""
    out = {}
    for name, _ in rec._fields_:
        v = getattr(rec, name)
        out.update({f'{name}.{k}': x for k, x in fields(v).items()} if isinstance(v, ctypes.Structure) else {name: v})
    return out


def _attn_cases():
    c = []
    for form in ATTN:
        rows = form in ('stream', 'pool')
        c += [(form, f, v, 'bad step shape') for f, v in (('shape.T', 0), ('shape.S', 1), ('shape.heads', 0), ('shape.B', 0 if rows else -1))]
        c += [(form, 'shape.D', 96, 'head_dim must be 64'), (form, 'shape.causal', 0, 'causal must be 1 or 2 (got 0)'), (form, 'shape.causal', 3, 'causal must be 1 or 2 (got 3)'),
              (form, 'T_total', 1025, 'T_total=1025 must be in'), (form, 'shape.dtype', F32X3, 'dtype must be TCOW_F32 or TCOW_BF16 (got 2)'),
              (form, 'cache_dtype', 7, 'cache_dtype must be TCOW_F32, TCOW_BF16 or TCOW_FP8E4M3 (got 7)'), (form, 'cache_dtype', -1, 'cache_dtype must be'),
              (form, 'cache_dtype', F32X3, 'cache_dtype must be'), (form, 'shape.dtype', BF16, 'cache_dtype TCOW_F32 is wider than the 16-bit storage')]
        # T_total below the chunk length is refused in the rows form (a chunk must fit into the cache); the F frames of a ragged step may exceed it
        c += [(form, 'T_total', 2, 'T_total=2 must be in [3, 1024]')] if rows else [(form, 'T_total', 0, 'T_total=0 must be in [1, 1024]')]
        if not rows:
            c += [(form, f, v, 'a ragged step is one row of F frames of 1 <= n <= F sessions') for f, v in (('n_sessions', 7), ('n_sessions', -1), ('shape.B', 2))]
        if form in ('pool', 'ragged'):
            c += [(form, 'n_slots', 0, 'n_slots=0 must be >= 1'), (form, 'n_slots', -1, 'n_slots=-1 must be >= 1')]
        if form == 'paged':
            c += [(form, 'page_frames', v, f'page_frames={v} must be a power of two') for v in (3, -4, 2048)]
            c += [(form, 'n_pages', 0, 'n_pages=0 must be >= 1'), (form, 'pages_per_session', 4, 'pages_per_session=4 x page_frames=8 does not cover T_total=40'),
                  (form, 'pages_per_session', 0, 'does not cover T_total')]
        else:
            c += [(form, 'page_frames', 3, 'page_frames=3 must be a power of two' if form == 'ragged' else 'a paged cache (page_frames=3) serves ragged steps only')]
        if rows:                                                    # rows + paged: refused with a message of its own
            c += [(form, 'page_frames', 8, 'a paged cache (page_frames=8) serves ragged steps only')]
        # every pointer of the form.  (slot_rows of the pool form is none: without it the record is the stream, which is valid.  A ragged
        # contiguous step without slot_rows is refused here.)
        c += [(form, f, None, 'null pointer') for f, v in ATTN[form].items() if v == SOME and (form, f) != ('pool', 'slot_rows')]
    return c


def _cls_cases():
    c = []
    for form in CLS:
        c += [(form, 'n', 0), (form, 'n', -2), (form, 'S', 1), (form, 'D', 0), (form, 'D', 126), (form, 'F', 2) if form == 'ragged' else (form, 'c', 0)]
        c += [(form, 'n_slots', 0), (form, 'n_slots', -1)] if form != 'stream' else []
        c += [(form, f, None) for f, v in CLS[form].items() if v == SOME and (form, f) != ('pool', 'slot_rows')]
    return c


ATTN_CASES, CLS_CASES = _attn_cases(), _cls_cases()
_id = lambda case: f'{case[0]}-{case[1]}={case[2]}'


@pytest.mark.parametrize('fmt', BUILDS)
def test_null_args_are_refused_first(fmt):
    lib = _lib.lib(fmt)
    for entry in ('tcow_attn_temporal_step', 'tcow_cls_step'):
        assert getattr(lib, entry)(None, None) == -1                # TCOW_ERR_INVALID_ARG
        message = lib.tcow_last_error().decode()
        assert message.startswith(entry + ': ') and 'args' in message, message


@pytest.mark.parametrize('fmt', BUILDS)
@pytest.mark.parametrize('form,field,value,text', ATTN_CASES, ids=[_id(c) for c in ATTN_CASES])
def test_each_attention_check_refuses_with_its_text(fmt, form, field, value, text):
    lib = _lib.lib(fmt)
    status = lib.tcow_attn_temporal_step(None, ctypes.byref(attn_record(form, **{field: value})))
    message = lib.tcow_last_error().decode()
    assert status == -1, (form, field, value, status, message)      # refused by a check, never by a failed launch
    assert message.startswith('tcow_attn_temporal_step: ') and text in message, (form, field, value, message)
    with pytest.raises(_lib.TcowError, match='tcow_attn_temporal_step failed'):
        _lib.check(status, 'tcow_attn_temporal_step', lib)


@pytest.mark.parametrize('fmt', BUILDS)
@pytest.mark.parametrize('form,field,value', CLS_CASES, ids=[_id(c) for c in CLS_CASES])
def test_each_cls_check_names_the_entry_point_and_the_field(fmt, form, field, value):
    lib = _lib.lib(fmt)
    status = lib.tcow_cls_step(None, ctypes.byref(cls_record(form, **{field: value})))
    message = lib.tcow_last_error().decode()
    assert status == -1, (form, field, value, status, message)
    assert message.startswith('tcow_cls_step: ') and message.split(': ', 1)[1].split()[0] == field, (form, field, value, message)
    with pytest.raises(_lib.TcowError, match='tcow_cls_step failed .*' + field):
        _lib.check(status, 'tcow_cls_step', lib)


def test_the_cases_differ_from_their_forms_valid_record_in_the_named_field_only():
    """(what the valid records are: every case above changes one of them in the named place, so the message can only come from that check)"""
    for form, field, value, _ in ATTN_CASES:
        good, bad = fields(attn_record(form)), fields(attn_record(form, **{field: value}))
        assert [k for k in good if good[k] != bad[k]] == [field], (form, field, value)
    for form, field, value in CLS_CASES:
        good, bad = fields(cls_record(form)), fields(cls_record(form, **{field: value}))
        assert [k for k in good if good[k] != bad[k]] == [field], (form, field, value)
    assert ctypes.sizeof(_lib.StreamAttnArgs) == 14 * 4 + 10 * 8 and ctypes.sizeof(_lib.StreamClsArgs) == 6 * 4 + 6 * 8
    # the forms are told apart by these fields alone
    forms = {k: fields(attn_record(k)) for k in ATTN}
    assert [(f['n_sessions'] != 0, f['page_frames'] != 0, f['slot_rows'] is not None) for f in forms.values()] == \
        [(False, False, False), (False, False, True), (True, False, True), (True, True, False)]
    assert {k: (v.get('first_rows') is not None, v.get('slot_rows') is not None) for k, v in CLS.items()} == \
        {'stream': (False, False), 'pool': (False, True), 'ragged': (True, True)}
