"""GPU: streaming steps in precision='bf16x3' with skinny_gemm=True (the steps' GEMMs through ops.gemm_nt_skinny_x3 where ops.skinny_plan_x3
routes them) against the same steps with skinny_gemm=False: stream, pool.step and pool.step_ragged, eager and graph mode; who calls the new entry
point and who never does.  The nets, clips and drivers are those of test_gpu_stream_skinny.py, restated: embed_dim 128 (K = 128 and 512, never
split: bit-identical) and embed_dim 768 (K = 768 and 3072, split), at 32 x 48 pixels."""
import pytest
import torch

from conftest import build_hip_seeker
from test_gpu_seeker import X3_TOL
from tcow_amd import ops, synth

pytestmark = pytest.mark.gpu

T, H, W = 4, 32, 48
NETS = {'d128': dict(embed_dim=128, depth=2, num_heads=2), 'd768': dict(embed_dim=768, depth=1, num_heads=12)}


@pytest.fixture(scope='module', autouse=True)
def _leave_no_scratch():
    """ops.workspace is a process-wide, grow-only cache that other tests look at: this module leaves none of its split-K scratch in it."""
    yield
    from tcow_amd import ops as o
    for k in [k for k in o._ws_cache if k[2] == 'nt_skinny']:
        del o._ws_cache[k]


def _net(which, precision='bf16x3', ca=1, seed=11):
    cfg = synth.seeker_config(num_total_frames=T, frame_height=H, frame_width=W, causal_attention=ca, **NETS[which])
    return build_hip_seeker(cfg, synth.make_state_dict(cfg, seed), precision).cuda().eval()


def _clips(n, seed=5):
    clip = synth.make_clip(n, T, H, W, seed=seed)
    rgb = torch.from_numpy(clip['rgb']).cuda()
    qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0)).cuda()
    if qm.shape[0] != n:
        qm = qm.expand(n, -1, -1, -1, -1).contiguous()
    return rgb, qm


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


@pytest.fixture
def spy(monkeypatch):
    calls = []
    real = ops.gemm_nt_skinny_x3

    def wrapped(A, Wt, out, *a, **kw):
        calls.append((A.shape[0], Wt.shape[0], A.shape[1], kw.get('split', 1)))
        return real(A, Wt, out, *a, **kw)

    monkeypatch.setattr(ops, 'gemm_nt_skinny_x3', wrapped)
    return calls


@pytest.mark.parametrize('which', ['d128', 'd768'])
def test_flagged_steps_agree_with_unflagged(cuda, spy, which):
    net = _net(which)
    rgb, qm = _clips(2)
    for run in (lambda **kw: list(_stream(net, rgb, qm, [1, 2, 1], **kw)), lambda **kw: _pool(net, rgb, qm, **kw), lambda **kw: _ragged(net, rgb, qm, **kw)):
        del spy[:]
        want = run(skinny_gemm=False)
        assert not spy                                                    # an unflagged step never calls the entry point
        got = run(skinny_gemm=True)
        assert spy                                                        # a flagged bf16x3 step does
        assert all(S == ops.skinny_plan_x3(M, N, K) and S >= 1 for M, N, K, S in spy)
        assert len(got) == len(want)
        if which == 'd128':
            assert all(s[3] == 1 for s in spy)                            # K = 128 and 512 never split: the 128 tile's bits
            assert all(torch.equal(g, w) for g, w in zip(got, want))
        else:
            assert any(s[2] == 768 for s in spy) and any(s[2] == 3072 for s in spy)
            for g, w in zip(got, want):
                assert float((g - w).abs().max()) < X3_TOL, float((g - w).abs().max())


def test_clip_forward_never_routes(cuda, spy):
    """The clip forward never takes the entry point, and after flagged steps it is what a fresh module computes."""
    net = _net('d768')
    rgb, qm = _clips(2)
    _stream(net, rgb, qm, [1, 1, 2], skinny_gemm=True)
    assert spy
    del spy[:]
    with torch.no_grad():
        m1, f1 = net(rgb, qm)
    assert not spy
    with torch.no_grad():
        m0, f0 = _net('d768')(rgb, qm)
    assert torch.equal(m1, m0) and torch.equal(f1, f0)


@pytest.mark.parametrize('which', ['d128', 'd768'])
def test_graph_mode_is_bit_identical_with_the_flag(cuda, which):
    net = _net(which)
    rgb, qm = _clips(2)
    split = [1, 1, 1, 1]                                                  # frames 1 .. 3 replay the graph captured at frame 0
    em, ef = _stream(net, rgb, qm, split, skinny_gemm=True)
    gm, gf = _stream(net, rgb, qm, split, skinny_gemm=True, graph=True)
    assert torch.equal(gm, em) and torch.equal(gf, ef)


def test_default_follows_the_precision(cuda, spy):
    """skinny_gemm=None: stream.SKINNY_GEMM_X3_DEFAULT in bf16x3, stream.SKINNY_GEMM_DEFAULT in bf16 -- for streams and pools."""
    from tcow_amd import stream
    assert isinstance(stream.SKINNY_GEMM_X3_DEFAULT, bool)
    x3, b16 = _net('d128'), _net('d128', 'bf16')
    assert x3.stream().skinny_gemm is stream.SKINNY_GEMM_X3_DEFAULT and x3.stream_pool(2).skinny_gemm is stream.SKINNY_GEMM_X3_DEFAULT
    assert b16.stream().skinny_gemm is stream.SKINNY_GEMM_DEFAULT and b16.stream_pool(2).skinny_gemm is stream.SKINNY_GEMM_DEFAULT
    rgb, qm = _clips(2)
    _stream(x3, rgb, qm, [2, 2])
    assert bool(spy) == stream.SKINNY_GEMM_X3_DEFAULT
    del spy[:]
    _stream(b16, rgb, qm, [2, 2])
    assert not spy                                                        # the 16-bit modes never take the bf16 x 3 entry point
