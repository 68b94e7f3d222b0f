"""CPU: Seeker.stream_pool() refuses what Seeker.stream() refuses (a frame's output would depend on later frames; modules it cannot run),
and a pool without a slot."""
import pytest

from conftest import build_hip_seeker
from stream_kit import _net
from tcow_amd import synth
from tcow_amd._lib import TcowError


@pytest.mark.parametrize('ca', [0, -1, 3])
def test_stream_pool_refuses_non_causal_attention(ca):
    with pytest.raises(TcowError, match='causal_attention'):
        _net(ca).eval().stream_pool(2)


def test_stream_pool_refuses_joint_space_time():
    with pytest.raises(TcowError, match='joint'):
        _net(0, 'joint_space_time').eval().stream_pool(2)


def test_stream_pool_refuses_training_mode():
    with pytest.raises(TcowError, match='training'):
        _net(1).train().stream_pool(2)


def test_stream_pool_refuses_forced_drop_masks():
    net = _net(2).eval()
    net.seeker.forced_drop_masks = {}
    with pytest.raises(TcowError, match='forced_drop_masks'):
        net.stream_pool(2)


def test_stream_pool_refuses_a_cpu_module():
    cfg = synth.seeker_config(num_total_frames=4, frame_height=32, frame_width=48, embed_dim=64, depth=1, num_heads=1, causal_attention=1)
    net = build_hip_seeker(cfg, synth.make_state_dict(cfg, 3), 'bf16').eval()
    for obj in (net, net.seeker):                               # both the Seeker wrapper and the QueryMaskTracker carry stream_pool()
        with pytest.raises(TcowError, match='CPU'):
            obj.stream_pool(capacity=2)


@pytest.mark.parametrize('capacity', [0, -1])
def test_stream_pool_refuses_a_capacity_below_one(capacity):
    net = _net(1).eval()
    for obj in (net, net.seeker):
        with pytest.raises(TcowError, match='capacity'):
            obj.stream_pool(capacity)
