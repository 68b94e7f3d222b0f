"""Host time of FusedAdamWClip.step() on the fast path, without a GPU: CPU tensors and the fake library of tests/optim_calls.py, whose step entry
point does nothing here (every entry-point name of old and new packages).  Two configurations: the bf16 cast path with module= (the trace kit's net)
and a plain parameter list.

    python tools/dev_optim_host_time.py leg                          one leg of the importable package: JSON {configuration: microseconds per step}
    python tools/dev_optim_host_time.py compare PARENT_DIR [OUT]     LEGS legs each of PARENT_DIR's package and of the tree, alternating process by
                                                                     process; writes / prints the medians and whether the tree's median exceeds the
                                                                     parent's by no more than the parent's own max - min
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS, WARMUP, CALLS, BATCH = 7, 300, 4000, 100
NAMES = ('tcow_adamw_clip_step', 'tcow_adamw_clip_step_scaled', 'tcow_adamw_clip_step_cast')


def leg():
    import pytest
    sys.path.append(ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import optim_calls as kit
    out = {}
    for name in ('module_bf16_cast', 'plain_list'):
        with pytest.MonkeyPatch.context() as mp:
            rec = kit.install(mp, lambda rec: {n: (lambda build, *args: 0) for n in NAMES})
            d = kit.module_optimizer(rec, [], 'bf16') if name == 'module_bf16_cast' else kit.plain_optimizer(rec, [])
            step = d.opt.step
            for _ in range(WARMUP):
                step()
            assert (d.opt._tiles is not None) == (name == 'module_bf16_cast')
            batches = []
            for _ in range(CALLS // BATCH):                         # a leg's figure is the median over its batches: a burst of another tenant of the host costs one batch
                t0 = time.perf_counter()
                for _ in range(BATCH):
                    step()
                batches.append((time.perf_counter() - t0) / BATCH * 1e6)
            out[name] = statistics.median(batches)
    print(json.dumps(out))


def compare(parent, path):
    runs = {'parent': [], 'tree': []}
    for _ in range(LEGS):
        for who, first in (('parent', os.path.abspath(parent)), ('tree', ROOT)):
            env = dict(os.environ, PYTHONPATH=first, OMP_NUM_THREADS='1')
            runs[who].append(json.loads(subprocess.check_output([sys.executable, os.path.abspath(__file__), 'leg'], env=env).decode().strip().split('\n')[-1]))
    doc = {'note': f'microseconds per FusedAdamWClip.step() on the fast path, CPU tensors, fake library; {LEGS} legs of {CALLS} calls after {WARMUP} each (a leg = the median of its batches of {BATCH}), parent and tree '
                   'alternating process by process; within_parent_spread: tree median - parent median <= parent max - min', 'host_step_us': {}}
    for name in runs['tree'][0]:
        p, t = [r[name] for r in runs['parent']], [r[name] for r in runs['tree']]
        doc['host_step_us'][name] = {'parent': {'median': statistics.median(p), 'legs': p, 'min': min(p), 'max': max(p)},
                                     'tree': {'median': statistics.median(t), 'legs': t, 'min': min(t), 'max': max(t)},
                                     'tree_minus_parent_us': statistics.median(t) - statistics.median(p), 'parent_spread_us': max(p) - min(p),
                                     'within_parent_spread': statistics.median(t) - statistics.median(p) <= max(p) - min(p)}
    text = json.dumps(doc, indent=1)
    if path:
        with open(path, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    if sys.argv[1:2] == ['leg']:
        leg()
    else:
        compare(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
