"""Writes tests/golden/stream_calls.json.gz: the host call trace of every case of tests/stream_calls.py, recorded on the CPU from the tcow_amd
package that is importable (the repository's, or the one PYTHONPATH puts first -- the fixture is generated from the commit BEFORE a change of
tcow_amd/stream.py and must not be regenerated to make a changed trace pass).

    python tools/make_stream_calls.py [output path]
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import stream_calls as kit  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else kit.FIXTURE
    traces = {}
    for name in kit.CASES:
        with pytest.MonkeyPatch.context() as mp:
            traces[name] = kit.run_case(name, mp)
        print(f'{name}: {len(traces[name])} entries')
    kit.save_fixture(traces, out)
    print(f'{out}: {os.path.getsize(out)} bytes, tcow_amd from {os.path.dirname(kit.stream.__file__)}')


if __name__ == '__main__':
    main()
