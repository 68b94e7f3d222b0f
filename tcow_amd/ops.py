"""Thin tensor-level wrappers over the libtcow_hip C ABI (include/tcow_hip.h).

PyTorch is used here only for device memory and streams: every function takes CUDA(HIP) tensors, passes raw
device pointers plus the current stream to the library and returns.  There is no fallback path: a missing or
failing library raises TcowError.
"""
import ctypes
import threading

import numpy as np
import torch

from . import _lib as L

F32, BF16 = L.TCOW_F32, L.TCOW_BF16
F32X3 = L.TCOW_F32X3      # GEMM wrappers only: f32 tensors, bf16 x 3 split products (csrc/gemm_x3.hip)
ACT_NONE, ACT_GELU, ACT_DGELU, ACT_GELU_DSAVE, ACT_MUL_AUX = L.ACT_NONE, L.ACT_GELU, L.ACT_DGELU, L.ACT_GELU_DSAVE, L.ACT_MUL_AUX


FP16 = 16                 # Python-side mode: the 16-bit mode (ABI dtype TCOW_BF16) of the binary16 build of the library, libtcow_hip_fp16.so


def tdtype(mode):
    return torch.bfloat16 if mode == BF16 else torch.float16 if mode == FP16 else torch.float32


def is16(mode):
    return mode in (BF16, FP16)


def _sel(mode):
    """(library, ABI dtype) of a mode: the binary16 build serves FP16 through its 16-bit dtype, everything else is the main library."""
    return (L.lib('fp16'), BF16) if mode == FP16 else (L.lib(), mode)


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_cur_device = getattr(torch._C, '_cuda_getDevice', None)


def _stream():
    """Raw hipStream_t of torch's current stream on the current device.  (torch.cuda.current_stream() builds a Python Stream object through
    four layers of device-index helpers: 8 us per call, ~430 calls per training step = 3.5 ms of the host's enqueue time.)"""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr() if t is not None else None


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.TcowError('libtcow_hip kernels need CUDA/HIP tensors (no CPU fallback on this path)')


def _gemm_args(dm, A, W, out, bias, row_scale, resid, act, aux, tile, bias2, row_scale2):
    M, K = A.shape
    return L.GemmArgs(M, W.shape[0], K, dm, A.data_ptr(), A.stride(0), W.data_ptr(), W.stride(0), out.data_ptr(), out.stride(0),
                      1 if out.dtype == torch.float32 else 0, _p(bias), _p(row_scale), _p(resid),
                      resid.stride(0) if resid is not None else 0, act, _p(aux), aux.stride(0) if aux is not None else 0, int(tile), _p(bias2), _p(row_scale2))


def gemm_nt(mode, A, W, out, bias=None, row_scale=None, resid=None, act=ACT_NONE, aux=None, tile=0, bias2=None, row_scale2=None, skinny=False):
    """out[M,N] = epilogue(A[M,K] @ W[N,K]^T); see tcow_gemm_nt. `out` dtype f32 or the mode's dtype.
    skinny=True (the streaming steps): a 16-bit product that skinny_plan routes goes to gemm_nt_skinny instead, a bf16 x 3 product that
    skinny_plan_x3 routes to gemm_nt_skinny_x3 when its tensors have that entry point's 16-byte alignment (a view that has not stays on
    tcow_gemm_nt, whose kernel has a scalar path); exact fp32 never routes."""
    if skinny and not tile:
        shape = A.shape[0], W.shape[0], A.shape[1]
        x3 = mode == F32X3 and _aligned16(A, W, out, bias, resid, aux, bias2)
        split = skinny_plan(*shape) if is16(mode) else skinny_plan_x3(*shape) if x3 else 0
        if split > 0:
            kw = dict(bias=bias, row_scale=row_scale, resid=resid, act=act, aux=aux, bias2=bias2, row_scale2=row_scale2, split=split)
            return gemm_nt_skinny(mode, A, W, out, **kw) if is16(mode) else gemm_nt_skinny_x3(A, W, out, **kw)
    _need_cuda(A, W, out)
    lib, dm = _sel(mode)
    a = _gemm_args(dm, A, W, out, bias, row_scale, resid, act, aux, tile, bias2, row_scale2)
    L.check(lib.tcow_gemm_nt(_stream(), ctypes.byref(a)), 'tcow_gemm_nt', lib)
    return out


SKINNY_SPLITS = (1, 2, 3, 4, 6, 8)


def _aligned16(*ts):
    """Every given tensor starts on a 16-byte boundary and, if 2-D, has a row pitch of whole 16 bytes (tcow_gemm_nt_skinny_x3's rule)."""
    return all(t is None or (t.data_ptr() % 16 == 0 and (t.dim() < 2 or t.stride(0) * t.element_size() % 16 == 0)) for t in ts)


def skinny_plan(M, N, K):
    """THE routing rule of the skinny-M NT GEMM (host arithmetic only): 0 = use tcow_gemm_nt, else the split S >= 1 of tcow_gemm_nt_skinny.
    Routed: K % 64 == 0 and fewer than 256 tiles of 128 x 128 -- where the 128 tile runs less than one round of the 256 CUs.  S is the smallest of
    SKINNY_SPLITS that starts at least 192 workgroups of 64 x 64 (three quarters of the CUs) while every slice keeps at least twelve 64-wide
    k-slices; if none does, the largest allowed.  Measured (profiles/gemm_skinny.json): the 64 tile itself is the gain; the
    second launch of a split costs about 4 us, more than a chain of fewer than twelve k-slices takes, so K = 768 never splits and K = 3072 splits
    only while its tiles leave most of the chip idle (M = 301: S = 4)."""
    M, N, K = int(M), int(N), int(K)
    if M < 1 or N < 1 or K < 64 or K % 64 or -(-M // 128) * -(-N // 128) >= 256:
        return 0
    tiles, nk = -(-M // 64) * -(-N // 64), K // 64
    allowed = [s for s in SKINNY_SPLITS if s == 1 or s <= nk // 12]
    for s in allowed:
        if tiles * s >= 192:
            return s
    return allowed[-1]


def _skinny_call(entry, mode, A, W, out, bias, row_scale, resid, act, aux, bias2, row_scale2, split):
    """What both skinny entry points do: `entry` of the mode's library on the arguments of gemm_nt, its slabs from workspace(tag='nt_skinny')."""
    _need_cuda(A, W, out)
    lib, dm = _sel(mode)
    split = int(split)
    a = _gemm_args(dm, A, W, out, bias, row_scale, resid, act, aux, 0, bias2, row_scale2)
    nbytes = lib.tcow_gemm_nt_skinny_workspace_bytes(a.M, a.N, split)
    ws = workspace(nbytes, A.device, 'nt_skinny') if nbytes > 0 else None
    L.check(getattr(lib, entry)(_stream(), ctypes.byref(a), split, _p(ws), ws.numel() if ws is not None else 0), entry, lib)
    return out


def gemm_nt_skinny(mode, A, W, out, bias=None, row_scale=None, resid=None, act=ACT_NONE, aux=None, bias2=None, row_scale2=None, split=1):
    """gemm_nt on 64 x 64 tiles with a deterministic split over K (tcow_gemm_nt_skinny; the 16-bit modes only).  split > 1 takes its [split, M, N]
    f32 slabs from workspace(tag='nt_skinny')."""
    if not is16(mode):
        raise L.TcowError('gemm_nt_skinny: the 16-bit modes only (fp32 and bf16x3 products go through gemm_nt)')
    return _skinny_call('tcow_gemm_nt_skinny', mode, A, W, out, bias, row_scale, resid, act, aux, bias2, row_scale2, split)


def skinny_plan_x3(M, N, K):
    """THE routing rule of the bf16 x 3 skinny-M NT GEMM (host arithmetic only): 0 = use tcow_gemm_nt, else the split S >= 1 of
    tcow_gemm_nt_skinny_x3.  Measured (profiles/gemm_skinny_x3.json and gemm_skinny_x3_small.json).
    Routed: K % 64 == 0 and N % 4 == 0 (what the entry point accepts), fewer than 256 tiles of 128 x 128 and at most 512 tiles of 64 x 64 --
    what the chip holds at once, two workgroups per CU; past that the 128 tile is as fast or faster (qkv at M = 1 201: 684 tiles, 33.2
    against 30.9 us; fc1: 912 tiles, 47.1 against 39.2).
    S: the largest of SKINNY_SPLITS that leaves every slice at least four 64-wide k-slices and keeps tiles x S within 256 workgroups for
    K < 1536 and within 512 from K = 1536: fc2 (K = 3072) S = 8 at M = 301, 40.9 -> 18.7 us, and S = 2 at M = 1 201, 46.7 -> 42.2; proj at
    M = 301 (60 tiles) S = 3, where the table's row is too noisy to rank the splits (all within the spread); every other K = 768 product of 180 tiles or more is fastest unsplit (its second launch and the slab pass
    cost more than the shorter chain saves).  At M = 14 ... 30 (12 ... 48 tiles) the K = 768 products are flat over S and fc2 gains 3 x from S = 8.
    Fewer than 8 tiles (toy nets) never split: an extrapolation, not measured -- such a step is bound by the host's launches, and a split
    adds one."""
    M, N, K = int(M), int(N), int(K)
    if M < 1 or N < 1 or N % 4 or K < 64 or K % 64 or -(-M // 128) * -(-N // 128) >= 256:
        return 0
    tiles, nk = -(-M // 64) * -(-N // 64), K // 64
    if tiles > 512:
        return 0
    if tiles < 8:
        return 1
    cap = 512 if nk >= 24 else 256
    return max(s for s in SKINNY_SPLITS if s == 1 or (s <= nk // 4 and tiles * s <= cap))


def gemm_nt_skinny_x3(A, W, out, bias=None, row_scale=None, resid=None, act=ACT_NONE, aux=None, bias2=None, row_scale2=None, split=1):
    """gemm_nt(F32X3, ...) on 64 x 64 tiles with a deterministic split over K (tcow_gemm_nt_skinny_x3): f32 tensors, 16-byte aligned, K % 64 == 0.
    split == 1 gives gemm_nt's bits; split > 1 takes its [split, M, N] f32 slabs from workspace(tag='nt_skinny'), the tag of gemm_nt_skinny."""
    return _skinny_call('tcow_gemm_nt_skinny_x3', F32X3, A, W, out, bias, row_scale, resid, act, aux, bias2, row_scale2, split)


class _Scratch(threading.local):          # the calling thread's scratch, gone with the thread
    def __init__(self):
        self.bufs, self.pinned = {}, {}                 # {(str(device), raw stream, tag): uint8 tensor}, {tag: tensor}


_scratch = _Scratch()


class pinned_workspace:
    """with pinned_workspace(tag, buf): workspace(..., tag) of this thread returns `buf` whatever the current stream is (and raises if it is too
    small).  A stream-graph capture runs on a side stream; pinning hands it the scratch that the eager step before it sized, so nothing is
    allocated inside the capture and the graph's owner knows the tensor the graph points into."""

    def __init__(self, tag, buf):
        self.tag, self.buf = tag, buf

    def __enter__(self):
        self.prev = _scratch.pinned.get(self.tag)
        _scratch.pinned[self.tag] = self.buf
        return self.buf

    def __exit__(self, *exc):
        if self.prev is None:
            del _scratch.pinned[self.tag]
        else:
            _scratch.pinned[self.tag] = self.prev


def workspace(nbytes, device, tag='default'):
    """Grow-only scratch buffer of the calling host thread per (device, STREAM, tag); workspace(0, device, tag) returns the one the thread has.
    Kernels on one stream run in order, so reuse within a stream is safe; two streams of one device never share scratch: the key carries torch's
    current stream, the one the launch that follows is made on.  Two host threads never share scratch either, not even on one stream (replicas of
    torch.nn.DataParallel placed on one device interleave their launches, and some scratch lives across two launches): each has its own table,
    which nothing counts or prunes.  A buffer that has to grow is replaced, and a thread's buffers go when the thread ends; neither frees memory
    under a running kernel: a thread's buffers were allocated under the stream they are used on, so their storage returns to torch's caching
    allocator, which keeps the blocks for that stream until the work queued on it has drained."""
    s = _scratch
    pin = s.pinned.get(tag)
    if pin is not None:
        if pin.numel() < nbytes:
            raise L.TcowError(f'workspace({tag!r}): the pinned buffer holds {pin.numel()} bytes, {nbytes} are needed')
        return pin
    key = (str(device), _stream(), tag)
    buf = s.bufs.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = s.bufs[key] = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=device)
    return buf


def workspace_view(tag):
    """{raw stream handle: tensor} of the calling thread's buffers under `tag`."""
    return {stream: buf for (_, stream, t), buf in _scratch.bufs.items() if t == tag}


def workspace_drop(tag):
    """Forget the calling thread's buffers under `tag`, on all streams."""
    _scratch.bufs = {key: buf for key, buf in _scratch.bufs.items() if key[2] != tag}


def gemm_tn(mode, dY, X, dW, bias_grad=None, accumulate=False):
    """dW[N,K] (+)= dY[M,N]^T @ X[M,K]; bias_grad[N] (+)= column sums of dY."""
    _need_cuda(dY, X, dW)
    M, N = dY.shape
    K = X.shape[1]
    lib, dm = _sel(mode)
    nbytes = lib.tcow_gemm_tn_workspace_bytes(M, N, K)
    ws = workspace(nbytes, dY.device, 'tn')
    L.check(lib.tcow_gemm_tn(_stream(), dm, M, N, K, dY.data_ptr(), dY.stride(0), X.data_ptr(), X.stride(0), dW.data_ptr(),
                             dW.stride(0), _p(bias_grad), int(accumulate), ws.data_ptr(), ws.numel()), 'tcow_gemm_tn', lib)
    return dW


def tn_group_max():
    """Most problems one grouped weight-gradient launch takes (tcow_gemm_tn_group_max)."""
    return int(L.lib().tcow_gemm_tn_group_max())


def gemm_tn_grouped(mode, problems):
    """Weight / bias gradients of several Linear layers in one call: problems = [(dY [M,N], X [M,K], dW [N,K] f32, bias_grad [N] or None), ...];
    an optional fifth element `accumulate` (default 0) adds the problem's result to dW / bias_grad instead of overwriting them.
    In bf16 mode problems that share M run as one grid (tcow_gemm_tn_grouped); the other modes loop inside the library."""
    n = len(problems)
    arr = (L.TnProblem * n)()
    for i, (dY, X, dW, db, *acc) in enumerate(problems):
        _need_cuda(dY, X, dW)
        arr[i] = L.TnProblem(dY.shape[0], dY.shape[1], X.shape[1], dY.data_ptr(), dY.stride(0), X.data_ptr(), X.stride(0), dW.data_ptr(), dW.stride(0), _p(db),
                             int(acc[0]) if acc else 0)
    lib, dm = _sel(mode)
    ws = workspace(lib.tcow_gemm_tn_grouped_workspace_bytes(dm, n, arr), problems[0][0].device, 'tn')
    L.check(lib.tcow_gemm_tn_grouped(_stream(), dm, n, arr, ws.data_ptr(), ws.numel()), 'tcow_gemm_tn_grouped', lib)


COLSUM_GROUP_MAX = 16    # tcow_colsum_group_max()


def colsum_grouped(mode, problems):
    """Bias gradients of Linear layers whose weight gradient is not wanted: problems = [(dY [M,N], out [N] f32), ...], out = column sums of dY;
    an optional third element `accumulate` (default 0) adds to out instead.  `mode` is the storage mode of the dY (tcow_colsum_grouped: N a
    multiple of 8 in the 16-bit modes, of 4 in f32 storage); up to 16 problems per call of the library, more are sent in chunks."""
    lib, dm = _sel(mode)
    for c0 in range(0, len(problems), COLSUM_GROUP_MAX):
        chunk = problems[c0:c0 + COLSUM_GROUP_MAX]
        n = len(chunk)
        arr = (L.ColsumProblem * n)()
        for i, (dY, out, *acc) in enumerate(chunk):
            _need_cuda(dY, out)
            arr[i] = L.ColsumProblem(dY.shape[0], dY.shape[1], dY.data_ptr(), dY.stride(0), out.data_ptr(), int(acc[0]) if acc else 0)
        ws = workspace(lib.tcow_colsum_grouped_workspace_bytes(dm, n, arr), chunk[0][0].device, 'colsum')
        L.check(lib.tcow_colsum_grouped(_stream(), dm, n, arr, ws.data_ptr(), ws.numel()), 'tcow_colsum_grouped', lib)


def sgemm_batched(problems, accumulate=False):
    """Small f32 products C (+)= A B, several per launch (tcow_sgemm_x3_batched).  problems = [(A, B, C), ...] with 2-D f32 tensors of ANY
    strides: A [M,K], B [K,N] (pass `.t()` views for transposed operands), C [M,N] row-major with unit column stride."""
    n = len(problems)
    arr = (L.SGemm * n)()
    for i, (A, B, C) in enumerate(problems):
        _need_cuda(A, B, C)
        M, K = A.shape
        N = B.shape[1]
        assert B.shape[0] == K and C.shape == (M, N) and C.stride(1) == 1 and A.dtype == B.dtype == C.dtype == torch.float32
        arr[i] = L.SGemm(M, N, K, A.data_ptr(), A.stride(0), A.stride(1), B.data_ptr(), B.stride(1), B.stride(0), C.data_ptr(), C.stride(0), 1 if accumulate else 0)
    L.check(L.lib().tcow_sgemm_x3_batched(_stream(), n, arr), 'tcow_sgemm_x3_batched')


def layernorm_fwd(mode, x, gamma, beta, out, mean=None, rstd=None, eps=1e-6):
    rows, D = x.shape
    lib, dm = _sel(mode)
    L.check(lib.tcow_layernorm_fwd(_stream(), dm, rows, D, x.data_ptr(), x.stride(0), gamma.data_ptr(), beta.data_ptr(), eps,
                                       out.data_ptr(), out.stride(0), _p(mean), _p(rstd)), 'tcow_layernorm_fwd', lib)
    return out


def layernorm_bwd(mode, dy, x, mean, rstd, gamma, dres, dx, dgamma=None, dbeta=None, accumulate=False, dx_cast=None, cast_scale=None,
                  colsum_out=None, colsum_scale=None, defer=None):
    """dx = dres + dLN(dy); dx_cast (mode dtype, optional) = dx * cast_scale[row]: the next input-gradient GEMM's operand;
    colsum_out [D] (optional) = sum over rows of colsum_scale[row] * dx[row].
    defer: a list -> the fold of the dgamma / dbeta (/ colsum) partial table is NOT launched; a job for layernorm_fold is appended instead (the
    table lives in its own workspace until then)."""
    rows, D = x.shape
    lib, dm = _sel(mode)
    if defer is not None and dgamma is not None:
        ws = workspace(lib.tcow_layernorm_bwd_workspace_bytes(D), x.device, 'ln_defer%d' % len(defer))
        defer.append((lib, ws, int(lib.tcow_layernorm_bwd_parts(rows, 1 if colsum_out is not None else 0)), D, dgamma, dbeta, colsum_out, bool(accumulate)))
        accumulate = int(accumulate) | 2
    else:
        ws = workspace(lib.tcow_layernorm_bwd_workspace_bytes(D), x.device, 'ln')
    L.check(lib.tcow_layernorm_bwd(_stream(), dm, rows, D, dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), mean.data_ptr(),
                                   rstd.data_ptr(), gamma.data_ptr(), _p(dres), dres.stride(0) if dres is not None else 0, dx.data_ptr(),
                                   dx.stride(0), _p(dgamma), _p(dbeta), int(accumulate), ws.data_ptr(), ws.numel(),
                                   _p(dx_cast), dx_cast.stride(0) if dx_cast is not None else 0, _p(cast_scale), _p(colsum_scale), _p(colsum_out)), 'tcow_layernorm_bwd', lib)
    return dx


def layernorm_fold(jobs):
    """The deferred dgamma / dbeta (/ colsum) folds of layernorm_bwd(..., defer=jobs): up to 16 per launch (tcow_layernorm_fold)."""
    for c0 in range(0, len(jobs), 16):
        chunk = jobs[c0:c0 + 16]
        lib = chunk[0][0]
        arr = (L.LnFoldJob * len(chunk))()
        for i, (_, ws, parts, D, dg, db, cs, acc) in enumerate(chunk):
            arr[i] = L.LnFoldJob(ws.data_ptr(), parts, D, dg.data_ptr(), db.data_ptr(), _p(cs), 1 if acc else 0)
        L.check(lib.tcow_layernorm_fold(_stream(), len(chunk), arr), 'tcow_layernorm_fold', lib)
    jobs.clear()


def attn_shape(mode, B, T, S, D, heads, causal):
    lib, dm = _sel(mode)
    sh = L.AttnShape(B, T, S, D, heads, int(causal), dm)
    sh.tcow_lib = lib              # which build of the library this shape's calls go to
    return sh


def attn_fwd(shape, spatial, qkv, out, lse=None):
    lib = shape.tcow_lib
    fn = lib.tcow_attn_spatial_fwd if spatial else lib.tcow_attn_temporal_fwd
    L.check(fn(_stream(), ctypes.byref(shape), qkv.data_ptr(), out.data_ptr(), _p(lse)), 'tcow_attn_fwd', lib)
    return out


def attn_bwd(shape, spatial, qkv, out, dout, lse, dqkv):
    lib = shape.tcow_lib
    ws = workspace(lib.tcow_attn_bwd_workspace_bytes(ctypes.byref(shape)), qkv.device, 'attn')
    fn = lib.tcow_attn_spatial_bwd if spatial else lib.tcow_attn_temporal_bwd
    L.check(fn(_stream(), ctypes.byref(shape), qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
               ws.data_ptr(), ws.numel()), 'tcow_attn_bwd', lib)
    return dqkv


def attn_probs(shape, spatial_rows, qkv, out, lse=None, pos=None):
    """The attention maps of one block from its qkv GEMM output [rows, 3D] (tcow_attn_probs), f32.  spatial_rows False: the temporal form,
    out [B, S-1, heads, T, T], lse [B*T*S, heads] as attn_fwd writes it.  True: the rows form -- pos, a device int32 table of nq query positions
    of the sequences attn_fwd(shape, True, ...) runs over; out [B*T, nq, heads, S], lse [B*T, nq, heads]."""
    _need_cuda(qkv, out, lse, pos)
    lib = shape.tcow_lib
    if pos is not None and (pos.dtype != torch.int32 or pos.dim() != 1 or not pos.is_contiguous()):
        raise L.TcowError(f'attn_probs: pos must be a contiguous int32 vector, got {pos.dtype} {tuple(pos.shape)}')
    if out.dtype != torch.float32 or not out.is_contiguous() or (lse is not None and (lse.dtype != torch.float32 or not lse.is_contiguous())):
        raise L.TcowError('attn_probs: out and lse must be contiguous float32 tensors')
    nq = pos.numel() if pos is not None else 0
    want = shape.B * shape.T * nq * shape.heads * shape.S if spatial_rows else shape.B * (shape.S - 1) * shape.heads * shape.T * shape.T
    if out.numel() != want or qkv.shape[0] != shape.B * shape.T * shape.S:
        raise L.TcowError(f'attn_probs: out must hold {want} floats and qkv {shape.B * shape.T * shape.S} rows, got {out.numel()} / {qkv.shape[0]}')
    if qkv.dim() != 2 or qkv.shape[1] != 3 * shape.D or not qkv.is_contiguous() or qkv.element_size() != (2 if shape.dtype == BF16 else 4):
        raise L.TcowError(f'attn_probs: qkv must be a contiguous [rows, {3 * shape.D}] tensor of the shape\'s storage type, got {qkv.dtype} {tuple(qkv.shape)}')
    want = shape.B * shape.T * (nq if spatial_rows else shape.S) * shape.heads
    if lse is not None and lse.numel() != want:
        raise L.TcowError(f'attn_probs: lse must hold {want} floats, got {lse.numel()}')
    args = L.AttnProbsArgs(shape, L.PROBS_ROWS if spatial_rows else L.PROBS_TEMPORAL, nq, _p(pos), qkv.data_ptr(), out.data_ptr(), _p(lse))
    L.check(lib.tcow_attn_probs(_stream(), ctypes.byref(args)), 'tcow_attn_probs', lib)
    return out


FP8 = L.TCOW_FP8E4M3      # cache_dtype of the attn_temporal_* wrappers only: a K / V cache of torch.float8_e4m3fn elements


STEP, STEP_PROBS = 'tcow_attn_temporal_step', 'tcow_attn_temporal_step_probs'        # the two entry points that take a tcow_stream_attn_args record


def _stream_attn(who, mode, B, T, S, D, heads, causal, cache_dtype, T_total, t0_rows, qkv, k_cache, v_cache, out, n_sessions=0, n_slots=0, slot_rows=None,
                 first_rows=None, c_rows=None, row_of_frame=None, page_frames=0, n_pages=0, pages_per_session=0, page_rows=None, symbol=STEP):
    """The call of the four attn_temporal_* wrappers (`who`): fills tcow_stream_attn_args (include/tcow_hip.h: which fields a form leaves 0 / None;
    the keywords are those) and calls tcow_attn_temporal_step of the mode's build.  `mode` is the attention mode: F32X3 (precision='bf16x3') stores f32 and runs as F32.
    symbol=STEP_PROBS: the same record to tcow_attn_temporal_step_probs -- `out` is then the maps, a contiguous f32 tensor of exactly
    F * (S-1) * heads * T_total elements (F = B * T flat frames), and the record's own out stays NULL.
    cache_dtype None = the storage type.  F32, BF16 (= the 16-bit type) or FP8: the caches must have the torch dtype it names -- torch.float8_e4m3fn;
    for BF16 the mode's 16-bit type, torch.bfloat16 under f32 storage (the main build serves it); torch.float32 -- and that refusal carries the
    wrapper's name.  A value or pair the library refuses (unknown, wider than the storage) is passed on for it to refuse, under its symbol."""
    lib, dm = _sel(mode)
    dm = F32 if dm == F32X3 else dm
    cq = dm if cache_dtype is None else int(cache_dtype)
    if cache_dtype is not None:
        want = torch.float8_e4m3fn if cq == FP8 else (tdtype(mode) if is16(mode) else torch.bfloat16) if cq == BF16 else \
            torch.float32 if cq == F32 and not is16(mode) else None
        if want is not None and (k_cache.dtype != want or v_cache.dtype != want):
            raise L.TcowError(f'{who}: cache_dtype={cq} needs {want} caches, got {k_cache.dtype} / {v_cache.dtype}')
    probs = symbol == STEP_PROBS
    if probs:
        want = B * T * (S - 1) * heads * int(T_total)
        if not torch.is_tensor(out) or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != want:
            raise L.TcowError(f'{who}: probs must be a contiguous float32 tensor of F * (S-1) * heads * T_total = {want} elements, got '
                              f'{(out.dtype, tuple(out.shape), "contiguous" if out.is_contiguous() else "strided") if torch.is_tensor(out) else type(out).__name__}')
    args = L.StreamAttnArgs(L.AttnShape(B, T, S, D, heads, int(causal), dm), cq, int(T_total), int(n_sessions), int(n_slots), int(page_frames), int(n_pages),
                            int(pages_per_session), t0_rows.data_ptr(), _p(slot_rows), _p(first_rows), _p(c_rows), _p(row_of_frame), _p(page_rows),
                            qkv.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), None if probs else out.data_ptr())
    fn = getattr(lib, symbol)
    L.check(fn(_stream(), ctypes.byref(args), out.data_ptr()) if probs else fn(_stream(), ctypes.byref(args)), symbol, lib)
    return out


def _stream_cls(x, n, c, F, S, cls_cache, n_slots, t0_rows, slot_rows=None, first_rows=None, c_rows=None):
    """The call of the three cls_* wrappers: fills tcow_stream_cls_args and calls tcow_cls_step (f32 rows: the main build)."""
    args = L.StreamClsArgs(int(n), int(c), int(F), S, x.shape[1], int(n_slots), x.data_ptr(), cls_cache.data_ptr(), t0_rows.data_ptr(), _p(slot_rows),
                           _p(first_rows), _p(c_rows))
    L.check(L.lib().tcow_cls_step(_stream(), ctypes.byref(args)), 'tcow_cls_step')
    return x


def attn_temporal_cached(mode, B, c, S, D, heads, causal, T_total, t0_dev, qkv, k_cache, v_cache, out, cache_dtype=None, who='attn_temporal_cached', symbol=STEP):
    """Temporal attention of a c-frame chunk (qkv [B*c*S, 3D] -> out [B*c*S, D]) against the K / V cache [B, S-1, heads, T_total, 64] of the
    frames before t0 = t0_dev[0] (int32 device scalar); appends the chunk's K / V at t0 (tcow_attn_temporal_step, the stream of the rows form).
    cache_dtype (here and in the three wrappers below): None = caches in the storage type; F32 / BF16 / FP8 = caches of that element type, every
    key and value taken at its value rounded to it (the compact cache of tcow_attn_temporal_step)."""
    _need_cuda(qkv, k_cache, v_cache, out, t0_dev)
    return _stream_attn(who, mode, B, c, S, D, heads, causal, cache_dtype, T_total, t0_dev, qkv, k_cache, v_cache, out, symbol=symbol)


def cls_stream(x, B, c, S, cls_cache, t0_dev):
    """causal_attention == 1 in a stream: t0 == 0 -> tcow_cls_merge mode 1 + keep the row in cls_cache [B, D]; t0 > 0 -> cls_cache to slot 0."""
    return _stream_cls(x, B, c, 0, S, cls_cache, 0, t0_dev)


def attn_temporal_pool(mode, n, c, S, D, heads, causal, T_total, n_slots, t0_rows, slot_rows, qkv, k_cache, v_cache, out, cache_dtype=None, who='attn_temporal_pool',
                       symbol=STEP):
    """attn_temporal_cached for n rows that stand at different frames: row r attends at t0_rows[r] against block slot_rows[r] of the caches
    [n_slots, S-1, heads, T_total, 64] and appends there (int32 device tensors [n]; distinct slots -- the rows form of tcow_attn_temporal_step)."""
    _need_cuda(qkv, k_cache, v_cache, out, t0_rows, slot_rows)
    return _stream_attn(who, mode, n, c, S, D, heads, causal, cache_dtype, T_total, t0_rows, qkv, k_cache, v_cache, out, n_slots=n_slots,
                        slot_rows=slot_rows, symbol=symbol)


def cls_pool(x, n, c, S, cls_cache, n_slots, t0_rows, slot_rows):
    """cls_stream per row: t0_rows[r] == 0 -> merge (mode 1) and keep the row in cls_cache[slot_rows[r]] ([n_slots, D]); > 0 -> that row to slot 0."""
    _need_cuda(x, cls_cache, t0_rows, slot_rows)
    return _stream_cls(x, n, c, 0, S, cls_cache, n_slots, t0_rows, slot_rows)


def _ragged_tables(who, n, F, t0_rows, slot_rows, first_rows, c_rows, row_of_frame=None):
    """What a host can check of a ragged step's tables: on the device, int32, one entry per session (per frame: row_of_frame)."""
    if n < 1:                   # (0 sessions in the record says "rows form")
        raise L.TcowError(f'{who}: a ragged step is one row of F frames of 1 <= n <= F sessions (F={F} n={n})')
    for name, t, want in (('t0_rows', t0_rows, n), ('slot_rows', slot_rows, n), ('first_rows', first_rows, n), ('c_rows', c_rows, n),
                          ('row_of_frame', row_of_frame, F)):
        if t is None and name in ('row_of_frame', 'slot_rows'):         # (cls_ragged has no frame table, the paged attention no slot table)
            continue
        _need_cuda(t)
        if t.dtype != torch.int32 or t.dim() != 1 or t.numel() != want or not t.is_contiguous():
            raise L.TcowError(f'{who}: {name} must be a contiguous int32 tensor of {want} entries (n = {n} sessions, F = {F} frames), got '
                              f'{t.dtype} {tuple(t.shape)}')


def _ragged_rows(who, F, S, qkv, out):
    """The rows of a ragged attention step: all F frames of all sessions, flat (out None: the maps, whose size _stream_attn checks)."""
    if out is None:
        if qkv.shape[0] != F * S:
            raise L.TcowError(f'{who}: qkv must have F * S = {F * S} rows, got {qkv.shape[0]}')
    elif qkv.shape[0] != F * S or out.shape[0] != F * S:
        raise L.TcowError(f'{who}: qkv / out must have F * S = {F * S} rows, got {qkv.shape[0]} / {out.shape[0]}')


def attn_temporal_ragged(mode, n, F, S, D, heads, causal, T_total, n_slots, t0_rows, slot_rows, first_rows, c_rows, row_of_frame, qkv, k_cache, v_cache,
                         out, cache_dtype=None, who='attn_temporal_ragged', symbol=STEP):
    """attn_temporal_pool for n sessions that bring different numbers of frames: session r owns the flat frames first_rows[r] .. + c_rows[r] - 1 of
    the step's F frames (qkv [F*S, 3D] -> out [F*S, D]), row_of_frame[f] names the session of frame f (int32 device tensors [n] / [F]); one wave per
    frame, bit-identical per session to attn_temporal_pool (the ragged form of tcow_attn_temporal_step)."""
    _need_cuda(qkv, k_cache, v_cache, out)
    _ragged_tables(who, n, F, t0_rows, slot_rows, first_rows, c_rows, row_of_frame)
    _ragged_rows(who, F, S, qkv, out if symbol == STEP else None)
    return _stream_attn(who, mode, 1, F, S, D, heads, causal, cache_dtype, T_total, t0_rows, qkv, k_cache, v_cache, out, n_sessions=n,
                        n_slots=n_slots, slot_rows=slot_rows, first_rows=first_rows, c_rows=c_rows, row_of_frame=row_of_frame, symbol=symbol)


def attn_temporal_ragged_paged(mode, n, F, S, D, heads, causal, T_total, n_pages, page_frames, t0_rows, page_rows, first_rows, c_rows, row_of_frame, qkv,
                               k_pages, v_pages, out, cache_dtype=None, who='attn_temporal_ragged_paged', symbol=STEP):
    """attn_temporal_ragged on a paged cache: k_pages / v_pages [n_pages, S-1, heads, page_frames, 64], and instead of a slot session r brings row r
    of page_rows (int32 device tensor [n, pages_per_session]): entry q is the page of its frames q * page_frames .. + page_frames - 1.
    Bit-identical to attn_temporal_ragged on contiguous caches of the same contents (the paged layout of tcow_attn_temporal_step)."""
    _need_cuda(qkv, k_pages, v_pages, out, page_rows)
    _ragged_tables(who, n, F, t0_rows, None, first_rows, c_rows, row_of_frame)
    if page_rows.dtype != torch.int32 or page_rows.dim() != 2 or page_rows.shape[0] != n or page_rows.shape[1] < 1 or not page_rows.is_contiguous():
        raise L.TcowError(f'{who}: page_rows must be a contiguous int32 tensor of n = {n} rows of pages_per_session entries, got '
                          f'{page_rows.dtype} {tuple(page_rows.shape)}')
    _ragged_rows(who, F, S, qkv, out if symbol == STEP else None)
    if not page_frames:         # (0 in the record says "contiguous": refused here, in the words the library has for every other bad page size)
        raise L.TcowError(f'{who}: page_frames=0 must be a power of two in [1, 1024]')
    return _stream_attn(who, mode, 1, F, S, D, heads, causal, cache_dtype, T_total, t0_rows, qkv, k_pages, v_pages, out, n_sessions=n,
                        first_rows=first_rows, c_rows=c_rows, row_of_frame=row_of_frame, page_frames=page_frames, n_pages=n_pages,
                        pages_per_session=page_rows.shape[1], page_rows=page_rows, symbol=symbol)


STEP_FORMS = {'stream': attn_temporal_cached, 'pool': attn_temporal_pool, 'ragged': attn_temporal_ragged, 'paged': attn_temporal_ragged_paged}


def attn_temporal_step_probs(form, *args, cache_dtype=None):
    """The attention maps of one stream step against its K cache (tcow_attn_temporal_step_probs): `form` names the wrapper whose record this is --
    'stream' (attn_temporal_cached), 'pool', 'ragged', 'paged' -- and the arguments are that wrapper's, with the maps `probs`, a contiguous f32
    tensor of exactly F * (S-1) * heads * T_total elements ([F, S-1, heads, T_total], F flat frames in the step's row order), in the place of
    `out`.  The same host checks of tables and cache dtypes apply; the caches are only read, nothing is appended."""
    if form not in STEP_FORMS:
        raise L.TcowError(f'attn_temporal_step_probs: form={form!r} must be one of {sorted(STEP_FORMS)}')
    return STEP_FORMS[form](*args, cache_dtype=cache_dtype, who='attn_temporal_step_probs', symbol=STEP_PROBS)


def cls_ragged(x, n, F, S, cls_cache, n_slots, t0_rows, slot_rows, first_rows, c_rows):
    """cls_pool for sessions of different chunk lengths: x [F*S, D]; session r's frames are first_rows[r] .. + c_rows[r] - 1 (the ragged form of
    tcow_cls_step)."""
    _need_cuda(x, cls_cache)
    _ragged_tables('cls_ragged', n, F, t0_rows, slot_rows, first_rows, c_rows)
    if x.shape[0] != F * S:
        raise L.TcowError(f'cls_ragged: x must have F * S = {F * S} rows, got {x.shape[0]}')
    return _stream_cls(x, n, 0, F, S, cls_cache, n_slots, t0_rows, slot_rows, first_rows, c_rows)


def requery_mask(logits, src_off, threshold, mask, dst_rows, pixels):
    """The hand-offs of a rollover pool step (see tcow_requery_mask): for hand-off i, the plane of mask.shape[1] f32 elements at element
    src_off[i] (device int64 [n]) of `logits` (any shape, f32, contiguous) -> mask[dst_rows[i]] (f32 [n_dst, plane]) as 0.0 / 1.0 of
    `> threshold`, and its number of ones -> pixels[dst_rows[i]] (int32 [n_dst]); dst_rows device int32 [n].  Nothing comes back to the host."""
    _need_cuda(logits, src_off, mask, dst_rows, pixels)
    if logits.dtype != torch.float32 or mask.dtype != torch.float32 or not logits.is_contiguous() or not mask.is_contiguous() or mask.dim() != 2:
        raise L.TcowError('requery_mask: logits and mask must be contiguous f32 tensors, mask [n_dst, plane]')
    n, n_dst = src_off.numel(), mask.shape[0]
    if n < 1 or mask.numel() < 1:
        raise L.TcowError(f'requery_mask: n={n} hand-offs, mask {tuple(mask.shape)}: at least one hand-off, one row and a plane of one element')
    if src_off.dtype != torch.int64 or dst_rows.dtype != torch.int32 or dst_rows.numel() != n or not src_off.is_contiguous() or not dst_rows.is_contiguous():
        raise L.TcowError(f'requery_mask: src_off must be int64 [n], dst_rows int32 [n], both contiguous, got {src_off.dtype} {tuple(src_off.shape)} / '
                          f'{dst_rows.dtype} {tuple(dst_rows.shape)}')
    if pixels.dtype != torch.int32 or pixels.numel() != n_dst or not pixels.is_contiguous():
        raise L.TcowError(f'requery_mask: pixels must be a contiguous int32 tensor of n_dst = {n_dst} entries, got {pixels.dtype} {tuple(pixels.shape)}')
    L.check(L.lib().tcow_requery_mask(_stream(), n, mask.shape[1], logits.data_ptr(), logits.numel(), src_off.data_ptr(), float(threshold), mask.data_ptr(),
                                      dst_rows.data_ptr(), n_dst, pixels.data_ptr()), 'tcow_requery_mask')
    return mask, pixels


def im2col(mode, rgb, query, P, pretrained_norm, out):
    B, _, T, H, W = rgb.shape
    lib, dm = _sel(mode)
    L.check(lib.tcow_im2col(_stream(), dm, B, T, H, W, P, rgb.data_ptr(), query.data_ptr(), int(pretrained_norm), out.data_ptr()), 'tcow_im2col', lib)
    return out


def gather_frames(frames, frame_idx, src_y, src_x):
    """frames (C,Tv,H,W) uint8 / 4-byte CUDA tensor, int32 CUDA index tables -> (C,Tc,h,w) (see tcow_gather_frames)."""
    _need_cuda(frames, frame_idx, src_y, src_x)
    if frames.element_size() not in (1, 4) or not frames.is_contiguous():
        raise L.TcowError('gather_frames: contiguous tensor of 1- or 4-byte elements expected')
    for t in (frame_idx, src_y, src_x):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise L.TcowError('gather_frames: index tables must be contiguous int32 tensors')
    C, Tv, H, W = frames.shape
    out = torch.empty(C, frame_idx.numel(), src_y.numel(), src_x.numel(), dtype=frames.dtype, device=frames.device)
    L.check(L.lib().tcow_gather_frames(_stream(), frames.element_size(), C, Tv, H, W, frame_idx.numel(), src_y.numel(), src_x.numel(), frames.data_ptr(),
                                       frame_idx.data_ptr(), src_y.data_ptr(), src_x.data_ptr(), out.data_ptr()), 'tcow_gather_frames')
    return out


def resize_aa(frames, frame_idx, ys, xs, ymin, ysize, wy, ky, xmin, xsize, wx, kx, out_h, out_w):
    """frames (C,Tv,H,W) f32 CUDA tensor + the index / weight tables of tcow_amd.augs (int32 / f32 CUDA tensors) -> (C,Tc,out_h,out_w) f32
    (see tcow_resize_aa)."""
    _need_cuda(frames, frame_idx, ys, xs, ymin, ysize, wy, xmin, xsize, wx)
    if frames.dtype != torch.float32 or not frames.is_contiguous():
        raise L.TcowError('resize_aa: contiguous f32 frames expected')
    for t, dt in ((frame_idx, torch.int32), (ys, torch.int32), (xs, torch.int32), (ymin, torch.int32), (ysize, torch.int32), (xmin, torch.int32), (xsize, torch.int32),
                  (wy, torch.float32), (wx, torch.float32)):
        if t.dtype != dt or not t.is_contiguous():
            raise L.TcowError('resize_aa: tables must be contiguous int32 / float32 tensors')
    C, Tv, H, W = frames.shape
    out = torch.empty(C, frame_idx.numel(), out_h, out_w, dtype=torch.float32, device=frames.device)
    L.check(L.lib().tcow_resize_aa(_stream(), C, Tv, H, W, frame_idx.numel(), ys.numel(), xs.numel(), out_h, out_w, frames.data_ptr(), frame_idx.data_ptr(), ys.data_ptr(),
                                   xs.data_ptr(), ymin.data_ptr(), ysize.data_ptr(), wy.data_ptr(), int(ky), xmin.data_ptr(), xsize.data_ptr(), wx.data_ptr(), int(kx),
                                   out.data_ptr()), 'tcow_resize_aa')
    return out


def photometric(frames, frame_idx, rect, order, factors, taps, gray):
    """frames (3,Tv,H,W) f32 CUDA tensor in [0, 1], frame_idx int32 CUDA table, rect = (y0, x0, h, w) -> (3,Tc,h,w) f32: ColorJitter adjustments
    `order` (list of 0 brightness / 1 contrast / 2 saturation / 3 hue, may be empty) with `factors` = (brightness, contrast, saturation, hue),
    5-tap blur with the normalised `taps` (None: no blur), grayscale fold (see tcow_photometric)."""
    _need_cuda(frames, frame_idx)
    if frames.dtype != torch.float32 or not frames.is_contiguous() or frames.dim() != 4 or frames.shape[0] != 3:
        raise L.TcowError('photometric: contiguous (3, Tv, H, W) f32 frames expected')
    if frame_idx.dtype != torch.int32 or not frame_idx.is_contiguous():
        raise L.TcowError('photometric: frame_idx must be a contiguous int32 tensor')
    _, Tv, H, W = frames.shape
    y0, x0, h, w = (int(v) for v in rect)
    Tc = frame_idx.numel()
    lib = L.lib()
    nb = lib.tcow_photometric_workspace_bytes(Tc)
    ws = torch.empty(max(nb // 4, 1), dtype=torch.float32, device=frames.device)
    out = torch.empty(3, Tc, h, w, dtype=torch.float32, device=frames.device)
    ops_arr = (ctypes.c_int * 4)(*([int(o) for o in order] + [0] * (4 - len(order))))
    taps_arr = (ctypes.c_float * 5)(*([float(t) for t in taps] if taps is not None else [0.0] * 5))
    fb, fc, fs, fh = (float(v) for v in factors)
    L.check(lib.tcow_photometric(_stream(), Tv, H, W, Tc, y0, x0, h, w, frames.data_ptr(), frame_idx.data_ptr(), len(order), ops_arr, fb, fc, fs, fh,
                                 1 if taps is not None else 0, taps_arr, 1 if gray else 0, ws.data_ptr(), nb, out.data_ptr()), 'tcow_photometric')
    return out


def im2col_channels(mode, src, P, normalise, out):
    """src (B,C,T,H,W) f32 -> out [B*T*S, C*P*P] (see tcow_im2col_channels)."""
    B, C, T, H, W = src.shape
    lib, dm = _sel(mode)
    L.check(lib.tcow_im2col_channels(_stream(), dm, B, T, H, W, P, C, src.data_ptr(), int(normalise), out.data_ptr()), 'tcow_im2col_channels', lib)
    return out


def _col2im_operand(who, dA, rows, cols, inv_scale):
    if inv_scale is not None and (inv_scale.dtype != torch.float32 or inv_scale.numel() != 1):
        raise L.TcowError(f'{who}: inv_scale must be one f32 element on the device, got {inv_scale.dtype} {tuple(inv_scale.shape)}')
    if dA.dtype != torch.float32 or dA.dim() != 2 or dA.stride(1) != 1 or dA.shape[0] != rows or dA.shape[1] < cols:
        raise L.TcowError(f'{who}: dA must be an f32 matrix of {rows} rows and at least {cols} columns with unit column stride, got {dA.dtype} {tuple(dA.shape)}')


def _col2im_image(who, name, t, shape):
    if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous()):
        raise L.TcowError(f'{who}: {name} must be a contiguous f32 tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}')


def col2im(dA, B, T, H, W, P, pretrained_norm, d_rgb, d_query, inv_scale=None):
    """The adjoint of im2col: dA f32 [B*T*S, >= 4*P*P] (a row pitch of its own is fine) -> d_rgb (B,3,T,H,W) / d_query (B,1,T,H,W) f32, either may be
    None (not wanted: not written); inv_scale: device f32 scalar multiplied in, or None (see tcow_col2im)."""
    _need_cuda(dA, d_rgb, d_query, inv_scale)
    _col2im_operand('col2im', dA, B * T * ((H // P) * (W // P) + 1), 4 * P * P, inv_scale)
    _col2im_image('col2im', 'd_rgb', d_rgb, (B, 3, T, H, W)); _col2im_image('col2im', 'd_query', d_query, (B, 1, T, H, W))
    L.check(L.lib().tcow_col2im(_stream(), B, T, H, W, P, dA.data_ptr(), dA.stride(0), _p(d_rgb), _p(d_query), int(pretrained_norm), _p(inv_scale)), 'tcow_col2im')
    return d_rgb, d_query


def col2im_channels(dA, P, normalise, dst, inv_scale=None):
    """dA f32 [B*T*S, >= C*P*P] -> dst (B,C,T,H,W) f32 (see tcow_col2im_channels)."""
    _need_cuda(dA, dst, inv_scale)
    B, C, T, H, W = dst.shape
    _col2im_operand('col2im_channels', dA, B * T * ((H // P) * (W // P) + 1), C * P * P, inv_scale)
    _col2im_image('col2im_channels', 'dst', dst, (B, C, T, H, W))
    L.check(L.lib().tcow_col2im_channels(_stream(), B, T, H, W, P, C, dA.data_ptr(), dA.stride(0), int(normalise), _p(inv_scale), dst.data_ptr()), 'tcow_col2im_channels')
    return dst


def embed_fwd(x, B, T, S, cls, pos, time_embed):
    L.check(L.lib().tcow_embed_fwd(_stream(), B, T, S, x.shape[1], x.data_ptr(), cls.data_ptr(), pos.data_ptr(), time_embed.data_ptr()), 'tcow_embed_fwd')
    return x


def embed_bwd(g, B, T, S, dpos, dtime, accumulate=False):
    L.check(L.lib().tcow_embed_bwd(_stream(), B, T, S, g.shape[1], g.data_ptr(), dpos.data_ptr(), dtime.data_ptr(), int(accumulate)), 'tcow_embed_bwd')


def cls_merge(x, B, T, S, mode, backward=False, cast_mode=None, cast_out=None, cast_scale=None):
    """cast_out (backward only): the 16-bit / f32 operand copy of x to refresh for the rewritten slot-0 rows (tcow_cls_merge_bwd_cast)."""
    if cast_out is not None:
        lib, dm = _sel(cast_mode)
        L.check(lib.tcow_cls_merge_bwd_cast(_stream(), dm, B, T, S, x.shape[1], x.data_ptr(), mode, cast_out.data_ptr(), cast_out.stride(0), _p(cast_scale)), 'tcow_cls_merge_bwd_cast', lib)
        return x
    L.check(L.lib().tcow_cls_merge(_stream(), B, T, S, x.shape[1], x.data_ptr(), mode, int(backward)), 'tcow_cls_merge')
    return x


def unpatchify_pool_fwd(mode, pm, BT, Hp, Wp, P, C, st, pooled):
    lib, dm = _sel(mode)
    L.check(lib.tcow_unpatchify_pool_fwd(_stream(), dm, BT, Hp, Wp, P, C, st, pm.data_ptr(), pooled.data_ptr()), 'tcow_unpatchify_pool_fwd', lib)
    return pooled


def unpatchify_pool_bwd(mode, dpooled, BT, Hp, Wp, P, C, st, dpm):
    lib, dm = _sel(mode)
    L.check(lib.tcow_unpatchify_pool_bwd(_stream(), dm, BT, Hp, Wp, P, C, st, dpooled.data_ptr(), dpm.data_ptr()), 'tcow_unpatchify_pool_bwd', lib)
    return dpm


def upsample_fwd(pooled, B, T, C, h, w, st, bilinear, out):
    L.check(L.lib().tcow_upsample_fwd(_stream(), B, T, C, h, w, st, int(bilinear), pooled.data_ptr(), out.data_ptr()), 'tcow_upsample_fwd')
    return out


def upsample_bwd(dout, B, T, C, h, w, st, bilinear, dpooled):
    L.check(L.lib().tcow_upsample_bwd(_stream(), B, T, C, h, w, st, int(bilinear), dout.data_ptr(), dpooled.data_ptr()), 'tcow_upsample_bwd')
    return dpooled


AMAX_SLOTS = 64          # TCOW_AMAX_SLOTS of include/tcow_hip.h


def upsample_bwd_amax(dout, B, T, C, h, w, st, dpooled):
    """upsample_bwd (bilinear, stride 4, h, w > 4) that also returns max |dout| as a 0-dim f32 device tensor (see tcow_upsample_bwd_amax)."""
    bits = torch.zeros(AMAX_SLOTS, dtype=torch.int32, device=dout.device)           # TCOW_AMAX_SLOTS partial maxima (one atomic per workgroup, spread over the slots)
    L.check(L.lib().tcow_upsample_bwd_amax(_stream(), B, T, C, h, w, st, dout.data_ptr(), dpooled.data_ptr(), bits.data_ptr(), AMAX_SLOTS), 'tcow_upsample_bwd_amax')
    return dpooled, bits.view(torch.float32).amax()


def flags_fwd(x, BT, S, Wf, bf, flags):
    L.check(L.lib().tcow_flags_fwd(_stream(), BT, S, x.shape[1], Wf.shape[0], x.data_ptr(), Wf.data_ptr(), bf.data_ptr(), flags.data_ptr()), 'tcow_flags_fwd')
    return flags


def scale_unless_one(x, scale):
    """x *= scale (a 0-dim / 1-element f32 device tensor) in place, decided on the device: no memory traffic when scale == 1 (tcow_scale_unless_one)."""
    _need_cuda(x, scale)
    if x.dtype != torch.float32 or not x.is_contiguous() or scale.dtype != torch.float32 or scale.numel() != 1:
        raise L.TcowError('scale_unless_one: a contiguous f32 tensor and a one-element f32 scale')
    L.check(L.lib().tcow_scale_unless_one(_stream(), x.data_ptr(), x.numel(), scale.data_ptr()), 'tcow_scale_unless_one')
    return x


def scale_cast(mode, src, row_scale, dst):
    rows, D = src.shape
    lib, dm = _sel(mode)
    L.check(lib.tcow_scale_cast(_stream(), dm, rows, D, src.data_ptr(), src.stride(0), _p(row_scale), dst.data_ptr(), dst.stride(0)), 'tcow_scale_cast', lib)
    return dst


def droppath_rows(u, keep_p, mask0, B, T, S):
    """u (depth, B*(S-1) + B*T + B) f32 uniform draws, keep_p (depth,) f32, mask0 [B*T*S] f32 -> (4, depth, B*T*S) f32 row scales
    (temporal | spatial | MLP | temporal x mask0), see tcow_droppath_rows."""
    _need_cuda(u, keep_p, mask0)
    depth = u.shape[0]
    if u.shape[1] != B * (S - 1) + B * T + B or u.dtype != torch.float32 or not u.is_contiguous() or mask0.numel() != B * T * S:
        raise L.TcowError('droppath_rows: u must be contiguous f32 (depth, B*(S-1) + B*T + B), mask0 [B*T*S]')
    out = torch.empty(4, depth, B * T * S, dtype=torch.float32, device=u.device)
    L.check(L.lib().tcow_droppath_rows(_stream(), depth, B, T, S, u.data_ptr(), keep_p.data_ptr(), mask0.data_ptr(), out.data_ptr()), 'tcow_droppath_rows')
    return out


def cast_transpose(mode, W, Wc=None, Wt=None):
    N, K = W.shape
    lib, dm = _sel(mode)
    L.check(lib.tcow_cast_transpose(_stream(), dm, N, K, W.data_ptr(), _p(Wc), _p(Wt)), 'tcow_cast_transpose', lib)


def cast_transpose_batched(mode, table, n, total_tiles):
    """One launch for all operand copies; `table` is the uint8 device tensor of tcow_cast_desc records (see tcow_cast_transpose_batched)."""
    lib, dm = _sel(mode)
    L.check(lib.tcow_cast_transpose_batched(_stream(), dm, table.data_ptr(), int(n), int(total_tiles)), 'tcow_cast_transpose_batched', lib)


def _mask_loss_args(lib, ws_tag, logits, target, channel, pixel_w, frame_w, weighted_aot, aot_loss, topk_frac, loss_weight, loss_out, total, dlogits, focal):
    """The tcow_mask_loss_args record of channel `channel` of (BQ, C, T, H, W) f32 logits / targets, after the tensor checks; its workspace is the
    pinned one tagged ws_tag, sized for this job (the 4 B / pixel bit-pattern image only when the radix select runs)."""
    _need_cuda(logits, target, pixel_w, frame_w, loss_out, total, dlogits)
    BQ, C, T, H, W = logits.shape
    for t in (logits, target, dlogits):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.shape != logits.shape):
            raise L.TcowError('mask_loss: logits / target / dlogits must be contiguous f32 tensors of one shape')
    n_frames, frame_len = BQ * T, H * W
    if pixel_w is not None and (pixel_w.dtype != torch.float32 or not pixel_w.is_contiguous() or pixel_w.numel() != n_frames * frame_len):
        raise L.TcowError('mask_loss: pixel_w must be a contiguous f32 tensor with one weight per pixel')
    if frame_w is not None and (frame_w.dtype != torch.float32 or not frame_w.is_contiguous() or frame_w.numel() != n_frames):
        raise L.TcowError('mask_loss: frame_w must be a contiguous f32 tensor with one weight per frame')
    ws = workspace(lib.tcow_mask_loss_workspace_bytes_for(n_frames, frame_len, float(topk_frac), float(aot_loss)), logits.device, ws_tag)
    off = channel * T * frame_len * 4
    return L.MaskLossArgs(n_frames, frame_len, T, logits.data_ptr() + off, C * T * frame_len, target.data_ptr() + off, C * T * frame_len,
                          _p(pixel_w), _p(frame_w), 1 if weighted_aot else 0, float(aot_loss), float(topk_frac), float(loss_weight),
                          loss_out.data_ptr(), _p(total), (dlogits.data_ptr() + off) if dlogits is not None else None,
                          C * T * frame_len, ws.data_ptr(), ws.numel(), 1 if focal else 0)


def mask_loss(logits, target, channel, pixel_w=None, frame_w=None, weighted_aot=False, aot_loss=0.8, topk_frac=1.0,
              loss_weight=1.0, loss_out=None, total=None, dlogits=None, focal=False):
    """Channel `channel` of the TCOW mask objective on (BQ, C, T, H, W) f32 logits / targets (see tcow_mask_loss):
    writes loss_out[0], adds loss_weight * loss to total[0] and d(loss)/d(logits) into dlogits[:, channel]."""
    lib = L.lib()
    a = _mask_loss_args(lib, 'mask_loss', logits, target, channel, pixel_w, frame_w, weighted_aot, aot_loss, topk_frac, loss_weight, loss_out, total, dlogits, focal)
    L.check(lib.tcow_mask_loss(_stream(), ctypes.byref(a)), 'tcow_mask_loss')
    return loss_out


def mask_loss_channels(logits, target, jobs, aot_loss=0.8, topk_frac=1.0, total=None, dlogits=None, focal=False):
    """Several channels of the TCOW mask objective in ONE set of launches (tcow_mask_loss_batch).  jobs: up to 4 tuples
    (channel, pixel_w | None, frame_w | None, weighted_aot, loss_weight, loss_out[1]); `total` receives sum_j loss_weight_j * loss_j in job order."""
    lib = L.lib()
    arr = (L.MaskLossArgs * len(jobs))()
    for i, (channel, pixel_w, frame_w, weighted_aot, loss_weight, loss_out) in enumerate(jobs):
        arr[i] = _mask_loss_args(lib, 'mask_loss%d' % i, logits, target, channel, pixel_w, frame_w, weighted_aot, aot_loss, topk_frac, loss_weight, loss_out, total,
                                 dlogits, focal)            # (every job of a batch needs its own workspace)
    L.check(lib.tcow_mask_loss_batch(_stream(), arr, len(jobs)), 'tcow_mask_loss_batch')


def iou_counts(logits, target):
    """(..., H, W) f32 logits / targets -> int32 (..., 3): target area, intersection, union per frame (see tcow_iou_counts)."""
    _need_cuda(logits, target)
    if logits.shape != target.shape or logits.dtype != torch.float32 or target.dtype != torch.float32:
        raise L.TcowError('iou_counts: logits and target must be f32 tensors of one shape')
    lo = logits.contiguous(); tg = target.contiguous()
    frame_len = lo.shape[-1] * lo.shape[-2]
    out = torch.empty(lo.shape[:-2] + (3,), dtype=torch.int32, device=lo.device)
    L.check(L.lib().tcow_iou_counts(_stream(), lo.data_ptr(), tg.data_ptr(), lo.numel() // frame_len, frame_len, out.data_ptr()), 'tcow_iou_counts')
    return out


def _mask_outputs(B, Q, T, H, W, dev):
    """What both mask builders write: query_mask (B,Q,1,T,H,W) f32, target (B,Q,3,T,H,W) f32, snitch_occl_by_ptr (B,Q,1,T,H,W) u8, counts int32 [1 + 2Q]."""
    return (torch.empty(B, Q, 1, T, H, W, dtype=torch.float32, device=dev), torch.empty(B, Q, 3, T, H, W, dtype=torch.float32, device=dev),
            torch.empty(B, Q, 1, T, H, W, dtype=torch.uint8, device=dev), torch.empty(1 + 2 * Q, dtype=torch.int32, device=dev))


def build_masks(segm, div_segm, query_idx, front_idx, cont_idx, query_time):
    """segm (B,1,T,H,W) u8, div_segm (B,M,T,H,W) u8, query_idx (B,Q) int32, front_idx / cont_idx (B,Q,T) int32 (-1 = none).
    Returns query_mask (B,Q,1,T,H,W) f32, target (B,Q,3,T,H,W) f32, snitch_occl_by_ptr (B,Q,1,T,H,W) u8, counts int32 [1 + 2Q]
    (see tcow_build_masks)."""
    _need_cuda(segm, div_segm, query_idx, front_idx, cont_idx)
    B, _, T, H, W = segm.shape
    M = div_segm.shape[1]; Q = query_idx.shape[1]
    if segm.dtype != torch.uint8 or div_segm.dtype != torch.uint8 or not segm.is_contiguous() or not div_segm.is_contiguous():
        raise L.TcowError('build_masks: segmentation maps must be contiguous uint8 tensors')
    qm, tg, pt, counts = _mask_outputs(B, Q, T, H, W, segm.device)
    qi = query_idx.to(torch.int32).contiguous(); fi = front_idx.to(torch.int32).contiguous(); ci = cont_idx.to(torch.int32).contiguous()
    L.check(L.lib().tcow_build_masks(_stream(), B, Q, M, T, H * W, int(query_time), segm.data_ptr(), div_segm.data_ptr(), qi.data_ptr(), fi.data_ptr(),
                                     ci.data_ptr(), qm.data_ptr(), tg.data_ptr(), pt.data_ptr(), counts.data_ptr()), 'tcow_build_masks')
    return qm, tg, pt, counts


def build_query_masks(segm, div_segm, occl_fracs, dag, sel, query_time, front_occl_thres, outer_cont_thres, occluded_weight, occl_cont_zero_weight):
    """data_utils.py:414-510 for every query of the batch, the per-frame occluder / container decisions included (tcow_build_query_masks):
    segm (B,1,T,H,W) u8, div_segm (B,M,T,H,W) u8, occl_fracs (B,K,T,3) f32, dag (B,T,M,M,3) f32, sel (B,Q) int64 queried instances.
    Returns a dict: query_mask (B,Q,1,T,H,W) f32, target (B,Q,3,T,H,W) f32, snitch_occl_by_ptr (B,Q,1,T,H,W) u8, counts int32 [1 + 2Q],
    ids (B,Q,T,2) u8, flags (B,Q,T,3) f32, sel_occl_fracs (B,Q,T,3) f32, frame_w (3,B,Q,T) f32 (snitch | occluder | container frame
    weights of loss.py:55-83, 285-308), front_idx / cont_idx (B,Q,T) int32."""
    _need_cuda(segm, div_segm, occl_fracs, dag, sel)
    B, _, T, H, W = segm.shape
    M = div_segm.shape[1]; K = occl_fracs.shape[1]; Q = sel.shape[1]
    if segm.dtype != torch.uint8 or div_segm.dtype != torch.uint8 or not segm.is_contiguous() or not div_segm.is_contiguous():
        raise L.TcowError('build_query_masks: segmentation maps must be contiguous uint8 tensors')
    if tuple(dag.shape) != (B, T, M, M, 3) or tuple(occl_fracs.shape[2:]) != (T, 3) or sel.dtype != torch.int64:
        raise L.TcowError('build_query_masks: occl_fracs (B,K,T,3), dag (B,T,M,M,3) and int64 sel (B,Q) expected')
    dev = segm.device
    of = occl_fracs.to(torch.float32).contiguous(); dg = dag.to(torch.float32).contiguous(); sl = sel.contiguous()
    n = B * Q * T
    qm, tg, pt, counts = _mask_outputs(B, Q, T, H, W, dev)
    idx = torch.empty(B * Q + 2 * n, dtype=torch.int32, device=dev)
    ids = torch.empty(B, Q, T, 2, dtype=torch.uint8, device=dev)
    fl = torch.empty(2, B, Q, T, 3, dtype=torch.float32, device=dev)         # flags | sel_occl_fracs (one allocation)
    fw = torch.empty(3, B, Q, T, dtype=torch.float32, device=dev)
    f32 = np.float32
    z = f32(occl_cont_zero_weight)
    has_w = f32(f32(1.0 - occl_cont_zero_weight) + z)                        # has * (1 - z) + z in f32, as the tensor expression rounds it
    L.check(L.lib().tcow_build_query_masks(_stream(), B, Q, K, M, T, H * W, int(query_time), segm.data_ptr(), div_segm.data_ptr(), of.data_ptr(), dg.data_ptr(),
                                           sl.data_ptr(), float(f32(front_occl_thres)), float(f32(front_occl_thres / 2.0)), float(f32(outer_cont_thres)),
                                           float(f32(float(occluded_weight))), float(z), float(has_w), idx.data_ptr(), ids.data_ptr(), fl[0].data_ptr(),
                                           fl[1].data_ptr(), fw.data_ptr(), qm.data_ptr(), tg.data_ptr(), pt.data_ptr(), counts.data_ptr()),
            'tcow_build_query_masks')
    return {'query_mask': qm, 'target': tg, 'snitch_occl_by_ptr': pt, 'counts': counts, 'ids': ids, 'flags': fl[0], 'sel_occl_fracs': fl[1], 'frame_w': fw,
            'front_idx': idx[B * Q:B * Q + n].view(B, Q, T), 'cont_idx': idx[B * Q + n:].view(B, Q, T)}


def iou_means(counts):
    """counts (n_seq, C, T, 3) int32 from iou_counts -> (mean f32 [6], count int32 [6]): eval/metrics.py:55-113 (see tcow_iou_means)."""
    _need_cuda(counts)
    if counts.dtype != torch.int32 or counts.dim() != 4 or counts.shape[-1] != 3 or not counts.is_contiguous():
        raise L.TcowError('iou_means: contiguous int32 (n_seq, C, T, 3) counts expected')
    n_seq, C, T, _ = counts.shape
    out = torch.empty(12, dtype=torch.float32, device=counts.device)
    cnt = out[6:].view(torch.int32)
    L.check(L.lib().tcow_iou_means(_stream(), counts.data_ptr(), n_seq, C, T, out.data_ptr(), cnt.data_ptr()), 'tcow_iou_means')
    return out[:6], cnt


def snitch_weights(target, snitch_occl_by_ptr, frame_w, pos_count, class_balancing=True, hard_negative_factor=3.0):
    """target (B,Q,3,T,H,W) f32 (channel 0 is used), snitch_occl_by_ptr (B,Q,1,T,H,W) u8, frame_w (B,Q,T) f32, pos_count int32 [>=1]
    -> (B,Q,T,H,W) f32 pixel weights of the track loss (see tcow_snitch_weights)."""
    _need_cuda(target, snitch_occl_by_ptr, frame_w, pos_count)
    B, Q, C, T, H, W = target.shape
    if not target.is_contiguous() or not snitch_occl_by_ptr.is_contiguous() or target.dtype != torch.float32 or snitch_occl_by_ptr.dtype != torch.uint8:
        raise L.TcowError('snitch_weights: target must be contiguous f32 and snitch_occl_by_ptr contiguous u8')
    out = torch.empty(B, Q, T, H, W, dtype=torch.float32, device=target.device)
    fw = frame_w.to(torch.float32).contiguous()
    lib = L.lib()
    ws = workspace(lib.tcow_snitch_weights_workspace_bytes(B * Q * T, H, W), target.device, 'snitch_w')
    L.check(lib.tcow_snitch_weights(_stream(), B * Q, T, H, W, target.data_ptr(), C * T * H * W, snitch_occl_by_ptr.data_ptr(), fw.data_ptr(), pos_count.data_ptr(),
                                    1 if class_balancing else 0, float(hard_negative_factor), out.data_ptr(), ws.data_ptr(), ws.numel()), 'tcow_snitch_weights')
    return out
