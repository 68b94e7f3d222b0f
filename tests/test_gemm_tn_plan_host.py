"""CPU: the host plan of the weight-gradient GEMM family (tcow_amd/csrc/gemm_tn_plan.h) and the LDS image of its 256-tile kernel.

  1. tools/tn_plan_check.cpp, built with the host compiler, sweeps shapes, dtypes and groups and asserts the plan's invariants (slices, stage
     multiples, bias-table rows written <= reserved, workspace regions disjoint, aligned and inside the total).
  2. The plan of every shape that tests/test_gpu_gemm_tn.py, tests/test_gpu_gemm_tn_k32.py and tests/test_gpu_gemm_x3_planes.py were chosen for: (kernel, slices requested, token
     rows per slice, slices, rows of the last slice).  A change of a slice rule that moves one of those shapes off the kernel form it was
     chosen for fails here, on the CPU, instead of silently un-testing that form.
  3. tcow_gemm_tn_workspace_bytes and tcow_gemm_tn_grouped_workspace_bytes of both library builds against tests/golden/tn_workspace_bytes.json,
     recorded by tools/make_tn_workspace_golden.py from the commit before the plan existed (host arithmetic: no GPU is touched).
  4. The LDS image (tcow_amd/csrc/gemm_tn_layout.h) enumerated lane by lane by tools/tn_layout_check.cpp."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT

FIXTURE = os.path.join(GOLDEN, 'tn_workspace_bytes.json')
BUILDS = ('bf16', 'fp16')
F32, BF16, F32X3 = 0, 1, 2
K128, K256_1, K256_2, KF32, KX3 = '128-tile', '256-tile SCHED 1', '256-tile SCHED 2', 'f32', 'x3'


def _cxx():
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler found'
    return cxx


def _build(tmp, name):
    exe = str(tmp / name)
    subprocess.run([_cxx(), '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'tcow_amd', 'csrc'), os.path.join(ROOT, 'tools', name + '.cpp'), '-o', exe],
                   check=True, capture_output=True, text=True, timeout=300)
    return exe


@pytest.fixture(scope='module')
def plan_check(tmp_path_factory):
    return _build(tmp_path_factory.mktemp('tn_plan'), 'tn_plan_check')


def _plan(exe, *args):
    """The `key=value` line tn_plan_check prints for one problem or one group, as a dict (integers where they are integers)."""
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    out = {}
    for item in run.stdout.strip().splitlines()[-1].split('  '):
        k, v = item.split('=')
        out[k] = int(v) if v.lstrip('-').isdigit() else v
    return out


# ---- 1
def test_plan_sweep(plan_check):
    run = subprocess.run([plan_check], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout[-4000:] + run.stderr[-2000:]


# ---- 2: (dtype, M, N, K) -> (kernel, slices requested, rows per slice, nz, rows of the last slice); ld = N, K unless given
PLANS = [
    # the row sweeps of test_gpu_gemm_tn.py, their end points and the shapes their docstrings name
    (BF16, 4800, 768, 768, (K256_2, 18, 320, 15, 320)),
    (BF16, 4801, 768, 768, (K256_2, 18, 320, 16, 1)),
    (BF16, 4863, 768, 768, (K256_2, 18, 320, 16, 63)),
    (BF16, 4864, 768, 768, (K256_2, 19, 256, 19, 256)),
    (BF16, 4865, 768, 768, (K256_2, 19, 320, 16, 65)),
    (BF16, 4930, 768, 768, (K256_2, 19, 320, 16, 130)),
    (BF16, 4096, 768, 768, (K256_2, 16, 256, 16, 256)),
    (BF16, 4224, 768, 768, (K256_2, 16, 320, 14, 64)),
    (BF16, 4096, 776, 520, (K256_1, 16, 256, 16, 256)),
    (BF16, 4097, 776, 520, (K256_1, 16, 320, 13, 257)),
    (BF16, 4160, 776, 520, (K256_1, 16, 320, 13, 320)),
    (BF16, 4161, 776, 520, (K256_1, 16, 320, 14, 1)),
    (BF16, 4230, 776, 520, (K256_1, 16, 320, 14, 70)),
    (BF16, 1, 136, 72, (K128, 1, 64, 1, 1)),
    (BF16, 140, 136, 72, (K128, 1, 192, 1, 140)),
    (BF16, 330, 136, 72, (K128, 1, 384, 1, 330)),
    (F32, 1, 136, 72, (KF32, 1, 16, 1, 1)),
    (F32, 330, 70, 50, (KF32, 1, 336, 1, 330)),
    (F32X3, 1, 136, 72, (KX3, 1, 32, 1, 1)),
    (F32X3, 330, 70, 50, (KX3, 1, 352, 1, 330)),
    # strided and poisoned operands, the engine form, the exact-workspace shapes
    (BF16, 4133, 768, 768, (K256_2, 16, 320, 13, 293)),
    (BF16, 4133, 776, 520, (K256_1, 16, 320, 13, 293)),
    (BF16, 513, 264, 136, (K128, 2, 320, 2, 193)),
    (BF16, 4160, 768, 256, (K128, 16, 320, 13, 320)),
    (BF16, 4133, 768, 256, (K128, 16, 320, 13, 293)),
    (BF16, 4200, 768, 768, (K256_2, 16, 320, 14, 40)),
    (F32, 513, 264, 136, (KF32, 2, 272, 2, 241)),
    (F32X3, 513, 264, 136, (KX3, 2, 288, 2, 225)),
    # bias-table edges
    (BF16, 4096, 8, 4224, (K128, 16, 256, 16, 256)),
    (BF16, 4096, 256, 16640, (K256_2, 3, 1408, 3, 1280)),
    (BF16, 2048, 8, 24704, (K128, 8, 256, 8, 256)),
    # test_gpu_gemm_tn_k32.py: the 32-token tails, the general path, full-range operands
    (BF16, 4097, 768, 768, (K256_2, 16, 320, 13, 257)),
    (BF16, 4159, 768, 768, (K256_2, 16, 320, 13, 319)),
    (BF16, 4113, 776, 768, (K256_1, 16, 320, 13, 273)),
    (BF16, 4129, 768, 776, (K256_1, 16, 320, 13, 289)),
    (BF16, 4129, 768, 768, (K256_2, 16, 320, 13, 289)),
]
# tests/test_gpu_gemm_x3_planes.py: the token sweep of the exact hi / lo checks of the bf16 x 3 kernel (tcow_tn_splits_x3: 768 / tiles slices, at least 256
# rows each), whose contraction stays within 1800 rows.  513: two slices of 288 rows = 9 k-slices of 32, an odd count; 1793: 7 slices, 65 rows in the last.
# (kept apart from PLANS: SINGLES below, and with it the recorded workspace fixture, stays as it is)
X3_PLANE_SWEEP = {1: (1, 32, 1, 1), 31: (1, 32, 1, 31), 32: (1, 32, 1, 32), 33: (1, 64, 1, 33), 64: (1, 64, 1, 64), 65: (1, 96, 1, 65), 255: (1, 256, 1, 255),
                  513: (2, 288, 2, 225), 1793: (7, 288, 7, 65)}
X3_PLANE_PLANS = [(F32X3, M, N, K, (KX3,) + want) for N, K in ((264, 136), (70, 50)) for M, want in X3_PLANE_SWEEP.items()]
# (dtype, M, N, K) -> (how the bias gradient is produced, bias-table rows written, rows_per_pk)
BIAS = [
    (BF16, 4096, 8, 4224, ('fused', 16 * 33 * 2, 1)),
    (BF16, 4096, 256, 16640, ('fused', 390, 1)),             # 3 slices x 65 k-tiles of 256 x 2
    (BF16, 2048, 8, 24704, ('colsum', 0, 1)),                # 8 x 193 x 2 = 3088 > 3072 table rows
    (BF16, 4133, 768, 768, ('fused', 13 * 3 * 2, 22)),
    (BF16, 513, 264, 136, ('fused', 2 * 2 * 2, 16)),
    (F32, 513, 264, 136, ('partials', 0, 0)),
    (F32X3, 513, 264, 136, ('partials', 0, 0)),
]


@pytest.mark.parametrize('dtype,M,N,K,want', PLANS + X3_PLANE_PLANS)
def test_plan_of_gpu_test_shape(plan_check, dtype, M, N, K, want):
    p = _plan(plan_check, 'one', dtype, M, N, K, 1)
    assert (p['kernel'].replace('_', ' '), p['splits'], p['mps'], p['nz'], p['last']) == want


@pytest.mark.parametrize('dtype,M,N,K,want', BIAS)
def test_bias_plan_of_gpu_test_shape(plan_check, dtype, M, N, K, want):
    p = _plan(plan_check, 'one', dtype, M, N, K, 1)
    assert (p['bias'], p['table_rows'], p['rows_per_pk']) == want
    assert _plan(plan_check, 'one', dtype, M, N, K, 0)['bias'] == 'none'


def test_strided_whole_tiles_keep_sched_2(plan_check):
    """ld = N + 8, K + 8 (the strided forms of the GPU tests) stays on SCHED 2; a product M ld of 2^29 or more does not."""
    assert _plan(plan_check, 'one', BF16, 4133, 768, 768, 1, 776, 776)['kernel'] == K256_2.replace(' ', '_')
    assert _plan(plan_check, 'one', BF16, 4133, 768, 768, 1, 1 << 17, 776)['kernel'] == K256_1.replace(' ', '_')


# ---- groups: name -> (dtype, [(M, N, K, ldy, ldx)]); the group sets of the two GPU test modules, the ViT-B step's, and groups that do not group
def _g(M, nks, pad=0):
    return [(M, N, K, N + pad, K + pad) for N, K in nks]


VITB_BLOCK = [(2304, 768), (768, 768), (768, 768), (2304, 768), (768, 768), (3072, 768), (768, 3072)]      # 153 tiles of 256 x 256
MIXED = [(768, 768), (776, 520), (256, 2304)]
GROUPS = {
    '7a': (BF16, _g(4133, MIXED, 8)),
    '7c': (BF16, _g(4133, [(2048, 2048), (1024, 4096), (4096, 1024), (2048, 2048)], 8)),
    '7d': (BF16, _g(4133, [(768, 768)] * 40, 8)),
    '7e group_max + 1': (BF16, _g(4133, [(768, 768)] * 41, 8)),
    '7f different M': (BF16, [(4133, 768, 768, 776, 776), (4200, 768, 768, 776, 776), (513, 264, 136, 272, 144)]),
    'k32 pair': (BF16, _g(4113, [(768, 768), (2304, 768)])),
    'k32 seven pairs': (BF16, _g(4113, [(768, 768), (2304, 768)] * 7)),
    'vitb block 27090': (BF16, _g(27090, VITB_BLOCK)),
    'vitb block 36120': (BF16, _g(36120, VITB_BLOCK)),
    'vitb four blocks 27090': (BF16, _g(27090, VITB_BLOCK * 4)),
    'vitb five blocks 27090': (BF16, _g(27090, VITB_BLOCK * 5)),
    'vitb five blocks 36120': (BF16, _g(36120, VITB_BLOCK * 5)),
    'vitb five blocks + five folds 36120': (BF16, _g(36120, VITB_BLOCK * 5 + [(768, 768)] * 5)),
    '7a f32': (F32, _g(4133, MIXED, 8)),
    '7a x3': (F32X3, _g(4133, MIXED, 8)),
    '7a odd pitch': (BF16, _g(4133, MIXED, 4)),
    'one problem': (BF16, _g(4133, [(768, 768)])),
    'small member': (BF16, _g(4133, [(768, 768), (768, 256)])),
}
# name -> (it runs as one grid, common slices requested)
GROUP_PLANS = {'7a': (1, 8), '7c': (1, 1), '7d': (1, 2), 'k32 pair': (1, 7), 'k32 seven pairs': (1, 1), 'vitb block 27090': (1, 5), 'vitb four blocks 27090': (1, 2),
               'vitb five blocks 27090': (1, 1), '7e group_max + 1': (0, 0), '7f different M': (0, 0), '7a f32': (0, 0), '7a x3': (0, 0), '7a odd pitch': (0, 0),
               'one problem': (0, 0), 'small member': (0, 0)}


def _group_args(dtype, probs):
    return ['group', dtype] + [v for p in probs for v in p]


@pytest.mark.parametrize('name', sorted(GROUP_PLANS))
def test_plan_of_group(plan_check, name):
    dtype, probs = GROUPS[name]
    p = _plan(plan_check, *_group_args(dtype, probs))
    assert (p['grouped'], p['splits']) == GROUP_PLANS[name]


def test_group_plan_details(plan_check):
    """7a: (8, 576, 8, 101), ragged member -> SCHED 1; 7c: one slice of all 4133 rows, SCHED 2; 7d: (2, 2112, 2, 2021); the k32 pair: (7, 640, 7, 273)."""
    want = {'7a': (K256_1, 576, 8, 101), '7c': (K256_2, 4160, 1, 4133), '7d': (K256_2, 2112, 2, 2021), 'k32 pair': (K256_2, 640, 7, 273),
            'k32 seven pairs': (K256_2, 4160, 1, 4113)}
    for name, w in want.items():
        p = _plan(plan_check, *_group_args(*GROUPS[name]))
        assert (p['kernel'].replace('_', ' '), p['mps'], p['nz'], p['last']) == w, name


# ---- 3
SINGLES = sorted({(M, N, K) for _, M, N, K, _ in PLANS} | {(M, N, K) for _, probs in GROUPS.values() for M, N, K, _, _ in probs} |
                 {(M, 70, 50) for M in (1, 140, 250, 330)} | {(250, 136, 72), (1, 8, 8), (255, 8, 8), (256, 3072, 3072), (100000, 3072, 3072), (16384, 128, 128)})


def _problem_table(L, probs):
    arr = (L.TnProblem * len(probs))()
    for i, (M, N, K, ldy, ldx) in enumerate(probs):
        arr[i] = L.TnProblem(M, N, K, 4096, ldy, 4096, ldx, 4096, K, None, 0)       # (the size function reads no pointer)
    return arr


def workspace_bytes(fmt):
    """What the size functions of one library build answer for SINGLES and GROUPS (the recorder and the test share this)."""
    from tcow_amd import _lib as L
    lib = L.lib(fmt)
    single = [[M, N, K, int(lib.tcow_gemm_tn_workspace_bytes(M, N, K))] for M, N, K in SINGLES]
    grouped = {name: int(lib.tcow_gemm_tn_grouped_workspace_bytes(dtype, len(probs), _problem_table(L, probs))) for name, (dtype, probs) in GROUPS.items()}
    return {'single': single, 'grouped': grouped}


@pytest.mark.parametrize('fmt', BUILDS)
def test_workspace_bytes_as_recorded(fmt):
    with open(FIXTURE) as f:
        doc = json.load(f)
    got = workspace_bytes(fmt)
    assert [r[:3] for r in doc[fmt]['single']] == [list(s) for s in SINGLES] and sorted(doc[fmt]['grouped']) == sorted(GROUPS), 'the fixture does not cover the cases'
    assert got['single'] == doc[fmt]['single']
    assert got['grouped'] == doc[fmt]['grouped']


def test_plan_total_is_the_library_size(plan_check):
    """The stand-alone program and the library include the same header: their totals agree with the recorded sizes."""
    with open(FIXTURE) as f:
        doc = json.load(f)['bf16']
    for M, N, K, nbytes in doc['single'][::7]:
        assert _plan(plan_check, 'one', BF16, M, N, K, 1)['total'] == nbytes, (M, N, K)
    for name, (dtype, probs) in GROUPS.items():
        assert _plan(plan_check, *_group_args(dtype, probs))['total'] == doc['grouped'][name], name


# ---- 4
def test_lds_layout_on_cpu(tmp_path):
    """tools/tn_layout_check.cpp includes the header the kernel uses and checks, over all lanes, that the loads write every element of a stage once,
    that every transpose read returns what the 16x16x32 operand layout demands, and that the transpose reads (per 32-lane half) and the 16-byte
    column-sum reads (per 16-lane group) are free of bank conflicts."""
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler found'
    exe = str(tmp_path / 'tn_layout_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'tcow_amd', 'csrc'), os.path.join(ROOT, 'tools', 'tn_layout_check.cpp'), '-o', exe],
                   check=True, capture_output=True, text=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
