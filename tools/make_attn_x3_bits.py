"""Writes tests/golden/attn_x3_bits.json: sha256 of out / lse / dqkv after every case of tests/attn_x3_bits.py -- ops.attn_fwd and ops.attn_bwd in
mode F32X3 on fixed inputs.  Needs the MI355X.  Recorded from the tcow_amd package that is importable WITH ITS OWN LIBRARIES (the repository's, or
the one PYTHONPATH puts first): the fixture comes from a built checkout of the commit before a change of the x3 attention kernels and is never
recorded from the tree it is meant to hold to the parent's bits.

    python tools/make_attn_x3_bits.py [output path]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import attn_x3_bits as kit  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'attn_x3_bits.json')
    doc = kit.run()
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    from tcow_amd import _lib
    print(f'{out}: {len(doc)} cases, {os.path.getsize(out)} bytes, tcow_amd from {os.path.dirname(_lib.__file__)}, library {_lib.LIB_PATH} '
          f'(ABI {_lib.lib().tcow_version()})')


if __name__ == '__main__':
    main()
