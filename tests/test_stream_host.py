"""CPU: Seeker.stream() refuses every configuration in which a frame's output would depend on later frames, and modules it cannot run."""
import pytest

from conftest import build_hip_seeker
from tcow_amd import synth
from tcow_amd._lib import TcowError


def _net(ca=1, attention_type='divided_space_time'):
    from tcow_amd.seeker import Seeker
    return Seeker(None, num_total_frames=4, frame_height=32, frame_width=48, network_depth=1, embed_dim=64, num_heads=1, causal_attention=ca,
                  attention_type=attention_type, drop_path_rate=0.0, precision='fp32')


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
