"""Host call-trace kit: the whole host side of SeekerStream, SeekerStreamPool and SeekerRolloverPool calls on CPU tensors -- sessions -> tables ->
step form -> page moves -> hand-offs -> which output slice is reported -- without a device or the library.

install(monkeypatch) puts five replacements in place (pytest's monkeypatch takes them out again):

  stream.check_streamable, stream._check_inputs   wrapped so that exactly their last refusal, the device check ("on the CPU" / "must be on the
                                                  stream device"), is swallowed; every other refusal propagates, in the order the code makes them.
  torch.cuda.device                               a null context.
  engine.run_forward                              records the step it is given (class, tables, skinny, cache shape / dtype, column 0 of the time
                                                  rows, the shapes of rgb / qm and a tag per flat frame of each) and returns mask logits and flags
                                                  whose value names (ordinal of the step, row, flat frame): CODE_STEP * (ordinal + 1) + CODE_ROW * row + frame.
  ops.requery_mask                                records (src_off, dst_rows, threshold) and copies the named plane into mask[dst], unthresholded,
                                                  so the next window's query tag says which step and frame made it.

The nets carry time_embed[0, t, :] = t, so column 0 of a step's time rows is the frame index of every flat frame.  The frames fed are coded
100 * session + global frame (rgb) and CODE_QM + the same (caller's query masks): a tag tells a caller's mask from an all-zero one (0.0) and
from a hand-off mask (>= CODE_STEP).  After every call the trace notes the state of the object; a refused call notes its message, and the state
after it, which test_stream_calls_host.py holds equal to the state before.

CASES / run_case() are pinned by tests/golden/stream_calls.json.gz (tools/make_stream_calls.py writes it, from the commit BEFORE a change of
tcow_amd/stream.py; it is not regenerated to make a changed trace pass).
"""
import contextlib
import gzip
import json
import os

import torch

from tcow_amd import engine, ops, stream
from tcow_amd._lib import TcowError
from tcow_amd.seeker import Seeker

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stream_calls.json.gz')
H, W = 32, 48
CODE_QM, CODE_STEP, CODE_ROW = 50000, 100000, 1000


def make_net(T=4):
    """The net of tests/test_stream_host.py (the smallest at which every branch is taken) with T frames, its time table naming the frame."""
    net = Seeker(None, num_total_frames=T, frame_height=H, frame_width=W, network_depth=1, embed_dim=64, num_heads=1, causal_attention=1,
                 attention_type='divided_space_time', drop_path_rate=0.0, precision='fp32').eval()
    with torch.no_grad():
        net.seeker.vit.time_embed.copy_(torch.arange(T, dtype=torch.float32)[None, :, None].expand_as(net.seeker.vit.time_embed))
    net.seeker.invalidate_param_cache()
    return net


def _swallow(fn, text, result):
    def wrapped(*args, **kwargs):
        try:
            return fn(*args, **kwargs)
        except TcowError as e:
            if text not in str(e):
                raise
            return result(*args, **kwargs)
    return wrapped


def install(monkeypatch):
    """The five replacements; returns the list that run_forward and requery_mask record into."""
    trace = []

    def run_forward(module, rgb, qm, params, save, stream=None, **kw):
        step, st = stream, stream.state
        trace.append(['forward', {
            'form': type(step).__name__, 'tables': [t.tolist() for t in step.tables], 'skinny': step.skinny,
            'cache': [list(st.k_cache.shape), str(st.k_cache.dtype)], 'frames': step.time_rows[:, 0].tolist(),
            'rgb': [list(rgb.shape), str(rgb.dtype), rgb[:, 0, :, 0, 0].tolist()], 'qm': [list(qm.shape), str(qm.dtype), qm[:, 0, :, 0, 0].tolist()]}])
        ordinal = sum(1 for e in trace if e[0] == 'forward')
        rows, F = rgb.shape[0], rgb.shape[2]
        code = CODE_STEP * ordinal + CODE_ROW * torch.arange(rows, dtype=torch.float32)[:, None] + torch.arange(F, dtype=torch.float32)[None, :]
        out_mask = code[:, None, :, None, None].expand(rows, module.output_channels, F, H, W).contiguous()
        flags = code[:, :, None].expand(rows, F, module.flag_channels).contiguous() if module.flag_channels > 0 else torch.zeros(0)
        return out_mask, flags, None

    def requery_mask(logits, src_off, threshold, mask, dst_rows, pixels):
        trace.append(['requery', {'src_off': src_off.tolist(), 'dst_rows': dst_rows.tolist(), 'threshold': threshold}])
        flat = logits.reshape(-1)
        for off, dst in zip(src_off.tolist(), dst_rows.tolist()):
            mask[dst] = flat[off:off + mask.shape[1]]

    monkeypatch.setattr(stream, 'check_streamable', _swallow(stream.check_streamable, 'on the CPU', lambda *a, **k: None))
    monkeypatch.setattr(stream, '_check_inputs', _swallow(stream._check_inputs, 'must be on the stream device', lambda who, m, device, clips, rows, rgb, qm: int(rgb.shape[2])))
    monkeypatch.setattr(torch.cuda, 'device', lambda device: contextlib.nullcontext())
    monkeypatch.setattr(engine, 'run_forward', run_forward)
    monkeypatch.setattr(ops, 'requery_mask', requery_mask)
    return trace


def coded(base, keys, g0s, c, channels):
    """(len(keys), channels, c, H, W) f32: row i, frame j holds base + 100 * keys[i] + g0s[i] + j."""
    keys = list(keys)
    v = torch.tensor([[base + 100 * k + g0 + j for j in range(c)] for k, g0 in zip(keys, g0s)], dtype=torch.float32).view(len(keys), c)
    return v[:, None, :, None, None].expand(len(keys), channels, c, H, W).contiguous()


def _out(t, flags=False):
    if t is None:
        return None
    if isinstance(t, (list, tuple)):
        return [_out(x, flags) for x in t]
    return [list(t.shape), (t[:, :, 0] if flags else t[:, 0, :, 0, 0]).tolist()]


class Driver:
    """Runs calls on one stream or pool and appends to the trace what each returned (or the refusal) and the state after it."""

    def __init__(self, trace, obj):
        self.trace, self.obj = trace, obj

    def state(self):
        o = self.obj
        if isinstance(o, stream.SeekerStream):
            return {'frames_done': o.frames_done}
        ids = sorted(o._slot)
        s = {'frames_done': {str(i): o.frames_done(i) for i in ids}}
        if o.page_frames is not None:
            s['pages_of'] = {str(i): list(o.pages_of(i)) for i in ids}
            s['pages_free'] = o.pages_free
        if isinstance(o, stream.SeekerRolloverPool):
            s['window'] = {str(i): o.window(i) for i in ids}
            s['retained'] = sorted(o._keep)
            s['handed'] = {str(i): float(o.requery_mask(i)[0, 0, 0, 0, 0]) for i in ids if i in o._last}
        return s

    def do(self, what, fn, result=lambda r: r):
        try:
            self.trace.append([what, result(fn())])
        except TcowError as e:
            self.trace.append([what, {'refused': str(e)}])
        self.trace.append(['state', self.state()])

    def _masks(self, ids, g0s, c, qm):
        return coded(CODE_QM, ids, g0s, c, 1) if qm else None

    def stream_step(self, c, qm=True):
        o = self.obj
        g0 = [o.frames_done] * o.B
        self.do('stream.step', lambda: o.step(coded(0, range(o.Bc), g0, c, 3), self._masks(range(o.B), g0, c, qm)),
                lambda r: [_out(r[0]), _out(r[1], True)])

    def step(self, ids, c, qm=True, rgb=None):
        o = self.obj
        known = [i if i in o._slot else 0 for i in ids]
        g0s = [o._done.get(i, 0) for i in ids]
        self.do('step', lambda: o.step(ids, coded(0, known, g0s, c, 3) if rgb is None else rgb, self._masks(known, g0s, c, qm)),
                lambda r: [_out(r[0]), _out(r[1], True)])

    def step_ragged(self, ids, cs, qms=True, n_rgbs=None, n_masks=None):
        """qms: True (every mask given), None, or a list of booleans (per entry: given or None)."""
        o = self.obj
        g0s = [o._done.get(i, 0) for i in ids]
        rgbs = [coded(0, [i], [g0], c, 3) for i, g0, c in zip(ids, g0s, cs)]
        given = [True] * len(ids) if qms is True else qms
        masks = None if given is None else [self._masks([i], [g0], c, q) for i, g0, c, q in zip(ids, g0s, cs, given)]
        rgbs = rgbs if n_rgbs is None else (rgbs * n_rgbs)[:n_rgbs]
        masks = masks if n_masks is None else (masks * n_masks)[:n_masks]
        self.do('step_ragged', lambda: o.step_ragged(ids, rgbs, masks), lambda r: [_out(r[0]), _out(r[1], True)])

    def call(self, name, *args):
        def result(r):
            return _out(r) if torch.is_tensor(r) and r.dim() == 5 else r.tolist() if torch.is_tensor(r) else list(r) if isinstance(r, tuple) else r
        self.do(name, lambda: getattr(self.obj, name)(*args), result)


# ------------------------------------------------------------------------------------------------------------------------- the pinned cases

def case_stream(tr, **kw):
    d = Driver(tr, make_net().stream(batch_size=2, queries_per_clip=2, **kw))
    d.stream_step(1)
    d.stream_step(2, qm=False)
    d.stream_step(1)
    d.stream_step(1)                                            # past the last frame
    d.call('reset')
    d.stream_step(3, qm=False)
    d.stream_step(2)                                            # frames 3..4 of 0..3
    d.do('stream.step', lambda: d.obj.step(torch.zeros(2, 3, 1, H, W + 1)))     # a refusal of _check_inputs other than the device


def case_pool(tr):
    d = Driver(tr, make_net().stream_pool(3))
    a = d.obj.open()
    d.step([a], 1)
    b = d.obj.open()
    d.step([b, a], 2, qm=False)
    c = d.obj.open()
    d.call('open')                                              # all slots taken
    d.step([c, a], 1)
    d.step([], 1)
    d.step([a, b, c, 7], 1)
    d.step([a, 7], 1)
    d.step([a, b, a], 1)
    d.step([b, a], 1)                                           # a has had its four frames
    d.step([b, c], 1, rgb=torch.zeros(2, 3, 1, H + 1, W))
    d.step_ragged([b, c], [1, 1], n_rgbs=1)
    d.step_ragged([b, c], [1, 1], n_masks=3)
    d.call('pages_of', b)                                       # a contiguous pool has no pages
    d.call('close', a)
    d.call('frames_done', a)
    e = d.obj.open()                                            # takes the slot a had
    d.step([e, b], 1)
    d.step([c, e, b], 1, qm=False)
    d.call('reset', b)
    d.step([b, c], 2)


def case_ragged(tr):
    d = Driver(tr, make_net().stream_pool(3))
    a, b, c = d.obj.open(), d.obj.open(), d.obj.open()
    d.step_ragged([a, b, c], [1, 2, 1], qms=None)
    d.step_ragged([b, a], [3, 1], qms=[False, True])            # b would pass its last frame
    d.step_ragged([a, c], [3, 1], qms=[False, True])
    d.step_ragged([b], [2])
    d.step_ragged([c, b], [2, 1], qms=[True, True])             # b is done
    d.step_ragged([c], [2], qms=[False])


def case_paged(tr, P, pages):
    d = Driver(tr, make_net().stream_pool(3, page_frames=P, pages=pages))
    a, b = d.obj.open(), d.obj.open()
    d.step([a, b], 1)
    d.step_ragged([b, a], [2, 1], qms=[True, False])            # b crosses a page boundary at P = 1 and 2
    d.step([a, b], 1)                                           # one more page than is free
    d.call('close', b)                                          # its pages return
    c = d.obj.open()
    d.step([c, a], 2, qm=False)                                 # the lowest free pages, b's among them; none is left
    d.step_ragged([c], [2], qms=None)
    d.call('reset', a)
    d.step_ragged([a, c], [1, 2])
    d.step([c], 1)                                              # past its last frame
    d.call('pages_of', 9)


# pages of a paged rollover case beyond one session's peak: the most with which some calls of the two sessions below are still refused
SPARE_PAGES = {(4, 1, 1): 2, (4, 1, 2): 0, (4, 2, 1): 3, (4, 2, 2): 2, (5, 2, 1): 3, (5, 2, 2): 3}


def case_rollover(tr, T, k, P, ragged):
    """Two sessions of a rollover pool over three windows and more: one frame per call, chunks of 2 and of s, a session that joins later, a call
    refused for pages (paged: the pool holds one session's peak and two pages), reset and close while two windows are live."""
    s, ceil = T - k, lambda a, b: -(-a // b)
    kw = {} if P is None else {'page_frames': P, 'pages': ceil(T, P) + ceil(k, P) + SPARE_PAGES[T, k, P]}
    d = Driver(tr, make_net(T).stream_pool(4, rollover=k, requery_threshold=0.25, **kw))
    o = d.obj

    def feed(ids, cs, qms=True):
        if ragged:
            d.step_ragged(ids, cs, qms)
        else:                                                   # step() takes one chunk length: the sessions one after the other where they differ
            for group in ([(ids, cs[0])] if len(set(cs)) == 1 else [([i], c) for i, c in zip(ids, cs)]):
                d.step(group[0], group[1], qm=qms is True)

    a = o.open()
    d.call('requery_mask', a)                                   # no hand-off yet
    d.call('requery_pixels', a)
    for _ in range(2 * s + k + 2):                              # one frame per call, into the third window
        feed([a], [1], qms=[True])
    d.call('requery_pixels', a)
    b = o.open()                                                # joins later, out of phase
    d.call('open')                                              # both slot pairs are taken
    feed([b], [1], qms=None)
    for _ in range(s + 2):                                      # chunks of 2: hand-off frames in the middle of a chunk and at its end
        feed([b, a], [2, 2] if s >= 2 else [1, 1], qms=[True, False] if ragged else True)
    feed([a, b], [s + 1, 1])                                    # more than s frames
    d.call('reset', a)                                          # mid-overlap
    for _ in range(3):
        feed([a, b], [s, 1], qms=None if ragged else True)
    d.call('pages_of', a)
    d.call('close', b)
    for _ in range(3):
        feed([a], [s])
    d.call('window', b)


def _cases():
    c = {'stream': case_stream, 'pool': case_pool, 'ragged': case_ragged}
    for P, pages in ((1, 6), (2, 3)):
        c[f'paged-P{P}'] = lambda tr, P=P, pages=pages: case_paged(tr, P, pages)
    for T, k in ((4, 1), (4, 2), (5, 2)):
        for P in (None, 1, 2):
            for ragged in (False, True):
                name = f"rollover-T{T}-k{k}-{'contiguous' if P is None else f'P{P}'}-{'step_ragged' if ragged else 'step'}"
                c[name] = lambda tr, T=T, k=k, P=P, ragged=ragged: case_rollover(tr, T, k, P, ragged)
    for cd in ('fp8', 'bf16'):
        c[f'cache-{cd}'] = lambda tr, cd=cd: case_stream(tr, cache_dtype=cd)
    return c


CASES = _cases()


def run_case(name, monkeypatch):
    """The trace of a case, in the form the fixture stores (after a JSON round trip)."""
    trace = install(monkeypatch)
    torch.manual_seed(0)
    CASES[name](trace)
    return json.loads(json.dumps(trace))


def save_fixture(traces, path=FIXTURE):
    blob = json.dumps(traces, separators=(',', ':'), sort_keys=True).encode()
    with open(path, 'wb') as f:
        with gzip.GzipFile(fileobj=f, mode='wb', mtime=0) as z:
            z.write(blob)


def load_fixture(path=FIXTURE):
    with gzip.open(path, 'rb') as z:
        return json.loads(z.read().decode())
