"""Writes tests/golden/optim_step_bits.json: sha256 of every parameter, moment and operand copy and the exact norm / skip count / loss-scale exponent
after each of the four steps of tests/optim_calls.py::bits_run, in bf16, fp16 and fp32.  Needs the MI355X.  Recorded from the tcow_amd package that is
importable WITH ITS OWN LIBRARIES (the repository's, or the one PYTHONPATH puts first): the fixture comes from a built checkout of the commit before
a change of the optimizer or its kernels and is never recorded from the tree it is meant to hold to the parent's bits.

    python tools/make_optim_bits.py [output path]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import optim_calls as kit  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else kit.BITS_FIXTURE
    doc = {p: kit.bits_run(p) for p in ('bf16', 'fp16', 'fp32')}
    for p, steps in doc.items():
        print(p, [(float.fromhex(s['grad_norm']), float.fromhex(s['skipped_steps']), float.fromhex(s['ls_log2']), s['tiles']) for s in steps])
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    from tcow_amd import _lib
    print(f'{out}: {os.path.getsize(out)} bytes, tcow_amd from {os.path.dirname(_lib.__file__)}, library {_lib.LIB_PATH} (ABI {_lib.lib().tcow_version()})')


if __name__ == '__main__':
    main()
