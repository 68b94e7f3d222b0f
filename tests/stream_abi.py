"""The ABI of the stream step since version 16, as the host tests of the stream family pin it: include/tcow_hip.h declares two records and two
entry points, tcow_amd/_lib.py mirrors them, both builds export them, and the eleven symbols they replaced are gone from all three."""
import ctypes
import os
import re

from tcow_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = 16
RECORDS = {'tcow_attn_temporal_step': ('tcow_stream_attn_args', 'StreamAttnArgs'), 'tcow_cls_step': ('tcow_stream_cls_args', 'StreamClsArgs')}
OLD = (['tcow_attn_temporal_%s%s_fwd' % (form, cq) for cq in ('', '_cq') for form in ('cached', 'pool', 'ragged', 'ragged_paged')] +
       ['tcow_cls_stream', 'tcow_cls_pool', 'tcow_cls_ragged'])
SCALARS = {'int': ctypes.c_int, 'long': ctypes.c_long, 'float': ctypes.c_float}
STRUCTS = {'tcow_attn_shape': _lib.AttnShape}


def header():
    """(the header, the header without comments)"""
    hdr = open(os.path.join(ROOT, 'include', 'tcow_hip.h')).read()
    return hdr, re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)


def header_fields(code, struct):
    """[(field, ctypes type)] of `typedef struct { ... } struct;` in declaration order: `int a, b;`, `const T* p;` (any pointer: c_void_p), `tcow_x s;`."""
    body = re.search(r'typedef\s+struct\s*\{([^}]*)\}\s*' + struct + r'\s*;', code)
    assert body, f'{struct} is not declared in tcow_hip.h'
    fields = []
    for decl in filter(None, (d.strip() for d in body.group(1).split(';'))):
        m = re.fullmatch(r'(?:const\s+)?(\w+)\s*(\*?)\s*(\w+(?:\s*,\s*\w+)*)', decl)
        assert m, f'{struct}: cannot read the declaration {decl!r}'
        base, star, names = m.groups()
        ctype = ctypes.c_void_p if star else SCALARS.get(base) or STRUCTS[base]
        fields += [(name.strip(), ctype) for name in names.split(',')]
    return fields


def check_version():
    hdr, _ = header()
    assert int(re.search(r'#define\s+TCOW_ABI_VERSION\s+(\d+)', hdr).group(1)) == ABI and _lib.ABI_VERSION == ABI


def check_header_and_records():
    """The header declares both records and both entry points; each ctypes.Structure has the header's fields, order and C types."""
    _, code = header()
    for entry, (struct, cls) in RECORDS.items():
        assert re.search(r'\bint\s+' + entry + r'\s*\(\s*void\s*\*\s*stream\s*,\s*const\s+' + struct + r'\s*\*\s*args\s*\)\s*;', code), f'{entry} is not declared'
        assert getattr(_lib, cls)._fields_ == header_fields(code, struct), (struct, cls)
        assert _lib.SIGNATURES[entry] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(getattr(_lib, cls))])


def check_builds_export():
    for fmt in ('bf16', 'fp16'):
        lib = _lib.lib(fmt)
        assert lib.tcow_version() == ABI
        for entry in RECORDS:
            assert hasattr(lib, entry), f'{entry} is not exported by the {fmt} build'
            assert getattr(lib, entry).argtypes == _lib.SIGNATURES[entry][1]


def check_old_symbols_are_gone(names=OLD):
    _, code = header()
    assert len(OLD) == 11 and set(names) <= set(OLD)
    for name in names:
        assert not re.search(r'\b' + name + r'\b', code), f'{name} is still declared in tcow_hip.h'
        assert name not in _lib.SIGNATURES
        for fmt in ('bf16', 'fp16'):
            assert not hasattr(_lib.lib(fmt), name), f'{name} is still exported by the {fmt} build'
