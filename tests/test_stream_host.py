"""CPU: Seeker.stream() refuses every configuration in which a frame's output would depend on later frames, and modules it cannot run."""
import pytest
import torch

from conftest import build_hip_seeker
from stream_kit import _net
from tcow_amd import engine, synth
from tcow_amd._lib import TcowError


@pytest.mark.parametrize('ca', [0, -1, 3])
def test_stream_refuses_non_causal_attention(ca):
    with pytest.raises(TcowError, match='causal_attention'):
        _net(ca).eval().stream()


def test_stream_refuses_joint_space_time():
    with pytest.raises(TcowError, match='joint'):
        _net(0, 'joint_space_time').eval().stream()


def test_stream_refuses_training_mode():
    with pytest.raises(TcowError, match='training'):
        _net(1).train().stream()


def test_stream_refuses_forced_drop_masks():
    net = _net(2).eval()
    net.seeker.forced_drop_masks = {}
    with pytest.raises(TcowError, match='forced_drop_masks'):
        net.stream()


def test_stream_refuses_a_cpu_module():
    cfg = synth.seeker_config(num_total_frames=4, frame_height=32, frame_width=48, embed_dim=64, depth=1, num_heads=1, causal_attention=1)
    net = build_hip_seeker(cfg, synth.make_state_dict(cfg, 3), 'bf16').eval()
    for obj in (net, net.seeker):                               # both the Seeker wrapper and the QueryMaskTracker carry stream()
        with pytest.raises(TcowError, match='CPU'):
            obj.stream(batch_size=1, queries_per_clip=1)


def test_chunk_geometry():
    """The chunk geometry counts the chunk's frames; the clip geometry is unchanged."""
    net = _net(1)
    g = net.seeker.geometry(2)
    gc = net.seeker.geometry(2, T=1)
    assert g['T'] == 4 and g['M'] == 2 * 4 * g['S']
    assert gc['T'] == 1 and gc['M'] == 2 * 1 * gc['S'] and gc['S'] == g['S']


def test_stream_step_mask0_equals_the_clip_path():
    """Whatever (B, T) a stream step has, its mask0 is the clip path's of the same (B, T), element for element."""
    m = _net(1).eval().seeker
    for B, T in ((1, 1), (2, 3), (3, 1), (1, 5)):
        g = m.geometry(B, T=T)
        mask0, _ = engine._row_vectors(m, g, False, stream_step=True)
        want, _ = engine._row_vectors(m, g, False)
        assert mask0.shape == (B * T * g['S'],) and torch.equal(mask0, want) and mask0.is_contiguous()


def test_stream_step_mask0_is_one_cache_entry_and_a_prefix():
    """The mask0 of stream steps is cached once per module: the longest vector asked for so far, shorter ones its prefixes."""
    m = _net(1).eval().seeker
    before = len(m._operands.copies)
    S = m.geometry(1)['S']
    seen = {}
    for B, F in ((1, 3), (1, 1), (1, 7), (2, 1), (1, 7), (3, 4), (1, 5)):
        mask0, _ = engine._row_vectors(m, m.geometry(B, T=F), False, stream_step=True)
        want, _ = engine._row_vectors(m, m.geometry(B, T=F), False)
        assert mask0.shape == (B * F * S,) and torch.equal(mask0, want) and mask0.is_contiguous()
        seen[B * F] = mask0.data_ptr()
    keys = [k for k in m._operands.copies if isinstance(k, tuple) and k[0] == 'mask0_frames']
    assert len(keys) == 1 and m._operands.copies[keys[0]].numel() == 12 * S
    assert len(m._operands.copies) == before + 1 + 6                              # (the six distinct (B, T) of the unshared form above, for comparison)
    assert seen[5] == seen[12] == m._operands.copies[keys[0]].data_ptr()          # a shorter vector after the longest one is its prefix
