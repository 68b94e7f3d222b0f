"""CPU: the argument checks of tcow_attn_probs (csrc/attention_probs.hip), against both builds of the library.  Every check returns before the
launch and none reads through a pointer, so no GPU is needed: each case differs from a valid record of its form in ONE field and must give
TCOW_ERR_INVALID_ARG and a message that starts with the entry point and names that field.  No case is valid: nothing launches."""
import ctypes

import pytest

from tcow_amd import _lib

BUILDS = ('bf16', 'fp16')
SOME = 0x1000                                   # a non-null address: no check reads through it
F32, BF16, F32X3 = _lib.TCOW_F32, _lib.TCOW_BF16, _lib.TCOW_F32X3
SHAPE = {'shape.B': 2, 'shape.T': 3, 'shape.S': 5, 'shape.D': 128, 'shape.heads': 2, 'shape.causal': 1, 'shape.dtype': BF16}
# the two forms (fields not named are 0 / NULL; lse may be NULL in both)
FORMS = {'temporal': dict(SHAPE, form=_lib.PROBS_TEMPORAL, qkv=SOME, out=SOME),
         'rows': dict(SHAPE, form=_lib.PROBS_ROWS, nq=3, pos=SOME, qkv=SOME, out=SOME, lse=SOME)}


def record(kind, **change):
    f = dict(FORMS[kind], **change)
    shape = _lib.AttnShape(**{k[6:]: f.pop(k) for k in list(f) if k.startswith('shape.')})
    return _lib.AttnProbsArgs(shape=shape, **f)


def fields(rec):
    out = {}
    for name, _ in rec._fields_:
        v = getattr(rec, name)
        out.update({f'{name}.{k}': x for k, x in fields(v).items()} if isinstance(v, ctypes.Structure) else {name: v})
    return out


def _cases():
    c = []
    for form in FORMS:
        c += [(form, 'shape.B', 0, 'must be >= 1'), (form, 'shape.B', -3, 'must be >= 1'), (form, 'shape.T', 0, 'must be >= 1'),
              (form, 'shape.S', 1, 'must be >= 2'), (form, 'shape.heads', 0, 'must be >= 1'),
              (form, 'shape.D', 96, 'must be heads * 64 = 128'), (form, 'shape.D', 192, 'must be heads * 64 = 128'),
              (form, 'shape.dtype', 3, 'must be TCOW_F32, TCOW_BF16 or TCOW_F32X3'), (form, 'shape.dtype', -1, 'must be TCOW_F32'),
              (form, 'form', 2, 'must be TCOW_PROBS_TEMPORAL or TCOW_PROBS_ROWS'), (form, 'form', -1, 'must be TCOW_PROBS_TEMPORAL'),
              (form, 'qkv', None, 'is NULL'), (form, 'out', None, 'is NULL')]
    c += [('temporal', 'shape.T', 1025, 'must be <= 1024 in the temporal form'), ('temporal', 'nq', 2, 'must be 0 in the temporal form'),
          ('temporal', 'nq', -1, 'must be 0 in the temporal form'), ('temporal', 'pos', SOME, 'must be NULL in the temporal form'),
          ('rows', 'nq', 0, 'must be >= 1 in the rows form'), ('rows', 'nq', -2, 'must be >= 1 in the rows form'),
          ('rows', 'pos', None, 'is NULL in the rows form')]
    return c


CASES = _cases()
_id = lambda case: f'{case[0]}-{case[1]}={case[2]}'


@pytest.mark.parametrize('fmt', BUILDS)
def test_null_args_are_refused_first(fmt):
    lib = _lib.lib(fmt)
    assert lib.tcow_attn_probs(None, None) == -1                    # TCOW_ERR_INVALID_ARG
    message = lib.tcow_last_error().decode()
    assert message.startswith('tcow_attn_probs: ') and 'args' in message, message


@pytest.mark.parametrize('fmt', BUILDS)
@pytest.mark.parametrize('form,field,value,text', CASES, ids=[_id(c) for c in CASES])
def test_each_check_names_the_entry_point_and_the_field(fmt, form, field, value, text):
    lib = _lib.lib(fmt)
    status = lib.tcow_attn_probs(None, ctypes.byref(record(form, **{field: value})))
    message = lib.tcow_last_error().decode()
    assert status == -1, (form, field, value, status, message)      # refused by a check, never by a failed launch
    assert message.startswith('tcow_attn_probs: ') and message.split(': ', 1)[1].split()[0] == field and text in message, (form, field, value, message)
    with pytest.raises(_lib.TcowError, match='tcow_attn_probs failed'):
        _lib.check(status, 'tcow_attn_probs', lib)


def test_every_check_has_its_own_text():
    """(two fields never share a message: the text alone tells which check refused)"""
    lib, seen = _lib.lib('bf16'), {}
    for form, field, value, _ in CASES:
        lib.tcow_attn_probs(None, ctypes.byref(record(form, **{field: value})))
        stem = ''.join(ch for ch in lib.tcow_last_error().decode() if not ch.isdigit() and ch != '-')
        assert seen.setdefault(stem, field) == field, (stem, field, seen[stem])


def test_the_cases_differ_from_their_forms_valid_record_in_the_named_field_only():
    for form, field, value, _ in CASES:
        good, bad = fields(record(form)), fields(record(form, **{field: value}))
        assert [k for k in good if good[k] != bad[k]] == [field], (form, field, value)
    assert ctypes.sizeof(_lib.AttnProbsArgs) == 10 * 4 + 4 * 8      # 7 + 2 ints, padded to 8 bytes, 4 pointers
    # what a form must leave 0 / NULL, and the one field that tells the forms apart
    t, r = fields(record('temporal')), fields(record('rows'))
    assert (t['form'], t['nq'], t['pos']) == (0, 0, None) and (r['form'], r['nq'] >= 1, r['pos'] is not None) == (1, True, True)
