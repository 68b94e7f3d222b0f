"""GPU: streaming steps with skinny_gemm=True (the steps' GEMMs through ops.gemm_nt_skinny where ops.skinny_plan routes a 16-bit product, through
ops.gemm_nt_skinny_x3 where ops.skinny_plan_x3 routes a bf16x3 one) against the same steps with skinny_gemm=False: stream, pool.step and
pool.step_ragged, eager and graph mode; who calls which entry point and who never does.  Two nets: embed_dim 128 (K = 128 and 512, never split)
and embed_dim 768 (K = 768, and K = 3072 with a split above 1), at 32 x 48 pixels."""
import pytest
import torch

from stream_kit import synth_clips, synth_net
from test_gpu_seeker import X3_TOL
from tcow_amd import ops

pytestmark = pytest.mark.gpu

T, H, W = 4, 32, 48
NETS = {'d128': dict(embed_dim=128, depth=2, num_heads=2), 'd768': dict(embed_dim=768, depth=1, num_heads=12)}
ENTRY = {'bf16': 'gemm_nt_skinny', 'fp16': 'gemm_nt_skinny', 'bf16x3': 'gemm_nt_skinny_x3', 'fp32': None}    # exact fp32 has no skinny kernel
ROUTED = [p for p in ENTRY if ENTRY[p]]


@pytest.fixture(scope='module', autouse=True)
def _leave_no_scratch():
    """ops.workspace keeps a thread's grow-only buffers for as long as the thread lives, and other tests look at them: this module leaves none of
    its split-K scratch behind."""
    yield
    from tcow_amd import ops as o
    o.workspace_drop('nt_skinny')


def _net(which, precision, ca=1, seed=11):
    return synth_net(precision, T, H, W, ca=ca, seed=seed, **NETS[which])


def _clips(n, seed=5):
    return synth_clips(n, T, H, W, seed)


def _stream(net, rgb, qm, split, **kw):
    st = net.stream(batch_size=rgb.shape[0], **kw)
    ms, fs, t = [], [], 0
    for c in split:
        m, f = st.step(rgb[:, :, t:t + c], qm[:, :, t:t + c])
        ms.append(m); fs.append(f); t += c
    return torch.cat(ms, 2), torch.cat(fs, 1)


def _pool(net, rgb, qm, **kw):
    """Two sessions out of phase: a leads by one frame, then both step together; all outputs in a fixed order."""
    pool = net.stream_pool(2, **kw)
    a, b = pool.open(), pool.open()
    outs = [pool.step([a], rgb[0:1, :, 0:1], qm[0:1, :, 0:1])]
    for t in range(1, 3):
        outs.append(pool.step([a, b], torch.cat([rgb[0:1, :, t:t + 1], rgb[1:2, :, t - 1:t]]), torch.cat([qm[0:1, :, t:t + 1], qm[1:2, :, t - 1:t]])))
    return [x for o in outs for x in o]


def _ragged(net, rgb, qm, **kw):
    """Session a brings 2 + 1 frames, b 1 + 3: two ragged steps of three and four frames."""
    pool = net.stream_pool(2, **kw)
    a, b = pool.open(), pool.open()
    m1, f1 = pool.step_ragged([a, b], [rgb[0:1, :, 0:2], rgb[1:2, :, 0:1]], [qm[0:1, :, 0:2], qm[1:2, :, 0:1]])
    m2, f2 = pool.step_ragged([b, a], [rgb[1:2, :, 1:4], rgb[0:1, :, 2:3]], [qm[1:2, :, 1:4], qm[0:1, :, 2:3]])
    return m1 + m2 + f1 + f2


def _agree(precision, got, want):
    """The unflagged run is the reference.  16-bit: the tolerances of test_stream_random_geometries_vs_oracle; fp32: the flag changes nothing;
    bf16x3: X3_TOL."""
    assert len(got) == len(want)
    if precision == 'fp32':
        assert all(torch.equal(g, w) for g, w in zip(got, want))
        return
    for g, w in zip(got, want):
        if precision == 'bf16x3':
            assert float((g - w).abs().max()) < X3_TOL, float((g - w).abs().max())
            continue
        std = float(w.std()) + 1e-6
        masks = w.dim() == 5
        tol = {('fp16', True): 0.00625 * std + 1e-5, ('fp16', False): 0.0015 * std + 2e-5, ('bf16', True): 0.05 * std + 1e-4, ('bf16', False): 0.012 * std + 2e-4}[(precision, masks)]
        assert float((g - w).abs().max()) < tol, (precision, masks, float((g - w).abs().max()), tol)


@pytest.fixture
def spy(monkeypatch):
    """Both public wrappers, wrapped: (M, N, K, split, wrapper's name) of every call."""
    calls = []

    def wrap(name, lead):                                                 # lead: the positional arguments in front of A (the mode)
        real = getattr(ops, name)

        def wrapped(*a, **kw):
            A, Wt = a[lead], a[lead + 1]
            calls.append((A.shape[0], Wt.shape[0], A.shape[1], kw.get('split', 1), name))
            return real(*a, **kw)

        monkeypatch.setattr(ops, name, wrapped)

    wrap('gemm_nt_skinny', 1)
    wrap('gemm_nt_skinny_x3', 0)
    return calls


@pytest.mark.parametrize('precision', ['bf16', 'fp16', 'fp32', 'bf16x3'])
@pytest.mark.parametrize('which', ['d128', 'd768'])
def test_flagged_steps_agree_with_unflagged(cuda, spy, which, precision):
    net = _net(which, precision)
    rgb, qm = _clips(2)
    for run in (lambda **kw: list(_stream(net, rgb, qm, [1, 2, 1], **kw)), lambda **kw: _pool(net, rgb, qm, **kw), lambda **kw: _ragged(net, rgb, qm, **kw)):
        del spy[:]
        want = run(skinny_gemm=False)
        assert not spy                                                    # an unflagged step never calls an entry point
        got = run(skinny_gemm=True)
        # a flagged step calls its precision's entry point and no other; fp32 has no skinny kernel and is not routed
        assert {s[4] for s in spy} == ({ENTRY[precision]} if ENTRY[precision] else set())
        if precision == 'bf16x3':
            assert all(S == ops.skinny_plan_x3(M, N, K) and S >= 1 for M, N, K, S, _ in spy)
            if which == 'd128':
                assert all(s[3] == 1 for s in spy)                        # K = 128 and 512 never split: the 128 tile's bits
                assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))
            else:
                assert any(s[2] == 768 for s in spy) and any(s[2] == 3072 for s in spy)
        elif which == 'd768' and precision != 'fp32':
            assert any(s[2] == 768 for s in spy) and any(s[3] > 1 and s[2] == 3072 for s in spy)      # (the measured rule splits K = 3072 only)
        _agree(precision, got, want)


@pytest.mark.parametrize('precision', ROUTED)
def test_default_and_clip_forward_do_not_route(cuda, spy, precision):
    """The clip forward never takes an entry point, and after flagged steps it is what a fresh module computes."""
    from tcow_amd import stream
    net = _net('d768', precision)
    rgb, qm = _clips(2)
    _stream(net, rgb, qm, [1, 1, 2], skinny_gemm=True)
    assert spy
    del spy[:]
    with torch.no_grad():
        m1, f1 = net(rgb, qm)
    assert not spy
    _stream(net, rgb, qm, [2, 2])                                         # the default: stream.SKINNY_GEMM_DEFAULT / SKINNY_GEMM_X3_DEFAULT
    assert bool(spy) == (stream.SKINNY_GEMM_X3_DEFAULT if precision == 'bf16x3' else stream.SKINNY_GEMM_DEFAULT)
    with torch.no_grad():
        m0, f0 = _net('d768', precision)(rgb, qm)
    assert torch.equal(m1, m0) and torch.equal(f1, f0)


@pytest.mark.parametrize('precision', ROUTED)
@pytest.mark.parametrize('which', ['d128', 'd768'])
def test_graph_mode_is_bit_identical_with_the_flag(cuda, which, precision):
    net = _net(which, precision)
    rgb, qm = _clips(2)
    split = [1, 1, 1, 1]                                                  # frames 1 .. 3 replay the graph captured at frame 0
    em, ef = _stream(net, rgb, qm, split, skinny_gemm=True)
    gm, gf = _stream(net, rgb, qm, split, skinny_gemm=True, graph=True)
    assert torch.equal(gm, em) and torch.equal(gf, ef)


def test_graph_keeps_the_workspace_it_was_captured_with(cuda):
    """ops.workspace replaces its tensor when it grows; a graph captured before that still owns the one its launches point into."""
    net = _net('d768', 'bf16')
    rgb, qm = _clips(2)
    st = net.stream(batch_size=2, graph=True, skinny_gemm=True)
    first = st.step(rgb[:, :, 0:1], qm[:, :, 0:1])
    ws = st._graphs[1]['ws']
    assert ws is not None and ws is ops.workspace(0, ws.device, 'nt_skinny')
    big = ops.workspace(ws.numel() * 4, ws.device, 'nt_skinny')           # a larger product on this stream: the cache moves on
    assert big is not ws and st._graphs[1]['ws'] is ws
    big.fill_(0xff)
    st.reset()
    again = st.step(rgb[:, :, 0:1], qm[:, :, 0:1])                        # frame 0 again: a replay, on the workspace of the capture
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])


def test_default_follows_the_precision(cuda, spy):
    """skinny_gemm=None: stream.SKINNY_GEMM_X3_DEFAULT in bf16x3, stream.SKINNY_GEMM_DEFAULT in bf16 -- for streams and pools."""
    from tcow_amd import stream
    assert isinstance(stream.SKINNY_GEMM_X3_DEFAULT, bool)
    x3, b16 = _net('d128', 'bf16x3'), _net('d128', 'bf16')
    assert x3.stream().skinny_gemm is stream.SKINNY_GEMM_X3_DEFAULT and x3.stream_pool(2).skinny_gemm is stream.SKINNY_GEMM_X3_DEFAULT
    assert b16.stream().skinny_gemm is stream.SKINNY_GEMM_DEFAULT and b16.stream_pool(2).skinny_gemm is stream.SKINNY_GEMM_DEFAULT
    rgb, qm = _clips(2)
    _stream(x3, rgb, qm, [2, 2])
    assert bool(spy) == stream.SKINNY_GEMM_X3_DEFAULT and all(s[4] == 'gemm_nt_skinny_x3' for s in spy)
    del spy[:]
    _stream(b16, rgb, qm, [2, 2])
    assert bool(spy) == stream.SKINNY_GEMM_DEFAULT and all(s[4] == 'gemm_nt_skinny' for s in spy)    # the 16-bit modes never take the bf16 x 3 entry point
