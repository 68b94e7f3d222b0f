"""CPU: the argument checks of tcow_col2im / tcow_col2im_channels (csrc/tokens.hip), against both builds of the library through ctypes, as
tests/test_glue_refusals_host.py does for the other glue entry points.  Every case is refused with TCOW_ERR_INVALID_ARG (-1) by a check in front of
the launch and tcow_last_error() names the entry point; no case reaches a launch, so no GPU is needed."""
import pytest

BUILDS = ('bf16', 'fp16')
Z, PTR = None, 4096                                                       # a null and a non-null pointer (never dereferenced)

# tcow_col2im(stream, B, T, H, W, P, dA, lda, d_rgb, d_query, pretrained_norm, inv_scale)
COL2IM = {
    'null dA': [Z, 1, 1, 16, 16, 4, Z, 64, PTR, PTR, 0, Z],
    'both outputs null': [Z, 1, 1, 16, 16, 4, PTR, 64, Z, Z, 0, Z],
    'P = 6': [Z, 1, 1, 18, 18, 6, PTR, 144, PTR, PTR, 0, Z],
    'H % P != 0': [Z, 1, 1, 18, 16, 4, PTR, 64, PTR, PTR, 0, Z],
    'W % P != 0': [Z, 1, 1, 16, 18, 4, PTR, 64, PTR, PTR, 0, Z],
    'B = 0': [Z, 0, 1, 16, 16, 4, PTR, 64, PTR, PTR, 0, Z],
    'T = 0': [Z, 1, 0, 16, 16, 4, PTR, 64, PTR, PTR, 0, Z],
    'lda < 4 P^2': [Z, 1, 1, 16, 16, 4, PTR, 60, PTR, PTR, 0, Z],
    'lda < 4 P^2, one output': [Z, 1, 1, 16, 16, 4, PTR, 16, Z, PTR, 0, Z],
    'lda % 4 != 0': [Z, 1, 1, 16, 16, 4, PTR, 66, PTR, PTR, 0, Z],
}
# tcow_col2im_channels(stream, B, T, H, W, P, C, dA, lda, normalise, inv_scale, dst)
CHANNELS = {
    'null dA': [Z, 1, 1, 16, 16, 4, 3, Z, 48, 0, Z, PTR],
    'null dst': [Z, 1, 1, 16, 16, 4, 3, PTR, 48, 0, Z, Z],
    'P = 6': [Z, 1, 1, 18, 18, 6, 3, PTR, 108, 0, Z, PTR],
    'H % P != 0': [Z, 1, 1, 18, 16, 4, 3, PTR, 48, 0, Z, PTR],
    'W % P != 0': [Z, 1, 1, 16, 18, 4, 3, PTR, 48, 0, Z, PTR],
    'B = 0': [Z, 0, 1, 16, 16, 4, 3, PTR, 48, 0, Z, PTR],
    'C = 0': [Z, 1, 1, 16, 16, 4, 0, PTR, 48, 0, Z, PTR],
    'lda < C P^2': [Z, 1, 1, 16, 16, 4, 3, PTR, 44, 0, Z, PTR],
    'lda % 4 != 0': [Z, 1, 1, 16, 16, 4, 1, PTR, 18, 0, Z, PTR],
}
CASES = [('tcow_col2im', k, v) for k, v in COL2IM.items()] + [('tcow_col2im_channels', k, v) for k, v in CHANNELS.items()]


@pytest.mark.parametrize('fmt', BUILDS)
@pytest.mark.parametrize('entry, what, args', CASES, ids=[f'{e}-{k}' for e, k, _ in CASES])
def test_refused_before_any_launch(fmt, entry, what, args):
    from tcow_amd import _lib
    lib = _lib.lib(fmt)
    assert len(args) == len(_lib.SIGNATURES[entry][1])
    status = getattr(lib, entry)(*args)
    message = lib.tcow_last_error().decode()
    assert status == -1, (what, status, message)
    assert message.startswith(entry + ':'), (what, message)
