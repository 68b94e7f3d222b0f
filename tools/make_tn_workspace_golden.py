"""Writes tests/golden/tn_workspace_bytes.json: what tcow_gemm_tn_workspace_bytes and tcow_gemm_tn_grouped_workspace_bytes of both library builds
answer for the shapes and groups listed in tests/test_gemm_tn_plan_host.py.  Both functions are host arithmetic: nothing touches a GPU.  The
fixture is recorded from the commit BEFORE a change of the weight-gradient GEMM's host rules and must not be regenerated to make a changed size pass.

    python tools/make_tn_workspace_golden.py [output path]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_gemm_tn_plan_host as kit  # noqa: E402


def main():
    from tcow_amd import _lib
    out = sys.argv[1] if len(sys.argv) > 1 else kit.FIXTURE
    doc = {'abi': _lib.ABI_VERSION}
    for fmt in kit.BUILDS:
        doc[fmt] = kit.workspace_bytes(fmt)
        print(f'{fmt}: {len(doc[fmt]["single"])} shapes, {len(doc[fmt]["grouped"])} groups')
    with open(out, 'w') as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write('\n')
    print(f'{out}: {os.path.getsize(out)} bytes, libraries from {os.path.dirname(_lib.LIB_PATH)}')


if __name__ == '__main__':
    main()
