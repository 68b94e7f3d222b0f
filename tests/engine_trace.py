"""Host trace kit: the launch schedule of tcow_amd.engine on CPU tensors, without the library.

install(monkeypatch) puts three replacements in place (pytest's monkeypatch takes them out again): tcow_amd._lib.lib returns a fake
library whose every entry point records its arguments and returns 0 (tcow_gemm_tn_group_max: 32, tcow_cast_desc_bytes and the optimizer's two: the record sizes),
ops._stream returns 0 and ops._need_cuda does nothing.  The schedule does not depend on the data and nothing syncs the host, so
SeekerFunction.apply(...) + .backward() and engine.run_forward(..., stream=step) run to the end; what they compute is garbage and is never
looked at.  Call the module through those two, not through Seeker.forward, which refuses CPU tensors.

A recorded call has two forms.  The NORMALISED one, [entry name, argument, ...], keeps every scalar; structs passed by reference and ctypes
arrays of structs (GemmArgs, AttnShape, TnProblem[], SGemm[], LnFoldJob[]) are unpacked into {field: value}.  What is a pointer is decided by
the declared types -- c_void_p in _lib.SIGNATURES and the c_void_p fields of the structs --, never by magnitude: a pointer becomes 'ptr',
a null one None (whether a bias, a row scale or an lse is passed is part of the schedule).  The RAW one keeps the non-null pointer values,
for tests about which buffer a call touches.

Limit: the normalised trace does not say WHICH buffer a pointer names, so it cannot see two operands swapped.  That is the job of the GPU
tests against the golden outputs.

CASES / run_case() are the schedules pinned by tests/golden/engine_trace.json.gz (tools/make_engine_trace.py writes it).
"""
import ctypes
import gzip
import json
import os

import torch

from tcow_amd import _lib, engine, ops, stream
from tcow_amd.seeker import Seeker

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'engine_trace.json.gz')
CAST_DESC_BYTES = 40                    # struct '<QQQiiii' of operands.OperandCache.refresh
ADAMW_CHUNK_BYTES, ADAMW_TILE_BYTES = 40, 56     # the optimizer's chunk and tile records (tcow_amd/optim_plan.py; tests/optim_calls.py runs it on this library)


def _struct(s, ptrs):
    out = {}
    for name, ftype in s._fields_:
        v = getattr(s, name)
        if ftype is ctypes.c_void_p:
            if v:
                ptrs.append(v)
            v = 'ptr' if v else None
        out[name] = v
    return out


def _argument(a, declared, ptrs):
    if hasattr(a, '_obj'):                                          # ctypes.byref(struct)
        return _struct(a._obj, ptrs)
    if isinstance(a, ctypes.Array):
        return [_struct(x, ptrs) if isinstance(x, ctypes.Structure) else x for x in a]
    if declared is ctypes.c_void_p:
        if a:
            ptrs.append(int(a))
        return 'ptr' if a else None
    return a


# The stream step's two entry points take one record each (tcow_stream_attn_args, tcow_stream_cls_args).  The fixture was recorded when every form
# of the step had a positional entry point of its own, and it is not regenerated: a recorded record is written out as that form's call -- the
# form's label (the former symbol), then these fields in this order -- and every field the form leaves out must be at rest (0 / NULL), so the
# pinned call and the record say the same thing.  (The record itself, field by field: tests/test_stream_attn_record_host.py.)
_ATTN_TAIL = ['qkv', 'k_cache', 'v_cache', 'out']
_RAGGED = ['first_rows', 'c_rows', 'row_of_frame']
STREAM_FORMS = {
    'cached': ['shape', 'T_total', 't0_rows'] + _ATTN_TAIL,
    'pool': ['shape', 'T_total', 'n_slots', 't0_rows', 'slot_rows'] + _ATTN_TAIL,
    'ragged': ['shape', 'n_sessions', 'T_total', 'n_slots', 't0_rows', 'slot_rows'] + _RAGGED + _ATTN_TAIL,
    'ragged_paged': ['shape', 'n_sessions', 'T_total', 'n_pages', 'page_frames', 'pages_per_session', 't0_rows', 'page_rows'] + _RAGGED + _ATTN_TAIL,
    'cls_stream': ['n', 'c', 'S', 'D', 'x', 'cls_cache', 't0_rows'],
    'cls_pool': ['n', 'c', 'S', 'D', 'x', 'cls_cache', 'n_slots', 't0_rows', 'slot_rows'],
    'cls_ragged': ['n', 'F', 'S', 'D', 'x', 'cls_cache', 'n_slots', 't0_rows', 'slot_rows', 'first_rows', 'c_rows'],
}


def _stream_form_call(name, rec, ptrs):
    """[form label, None (the stream), the form's fields ...] of a stream step record."""
    if name == 'tcow_cls_step':
        form = 'cls_ragged' if rec.first_rows or rec.c_rows else 'cls_pool' if rec.slot_rows else 'cls_stream'
        label, tail = 'tcow_' + form, []
    else:
        form = ('ragged_paged' if rec.page_frames else 'ragged') if rec.n_sessions else 'pool' if rec.slot_rows else 'cached'
        compact = rec.cache_dtype != rec.shape.dtype                # the storage type: the former entry points without a cache_dtype
        label, tail = f"tcow_attn_temporal_{form}{'_cq' if compact else ''}_fwd", [rec.cache_dtype] if compact else []
    fields, types = STREAM_FORMS[form], dict(rec._fields_)
    rest = {f: getattr(rec, f) for f in types if f not in fields and f != 'cache_dtype'}
    assert not any(rest.values()), (label, 'fields outside the form are set', rest)
    return [label, None] + [_struct(rec.shape, ptrs) if f == 'shape' else _argument(getattr(rec, f), types[f], ptrs) for f in fields] + tail


class Trace:
    """calls: the normalised calls in order.  events: ('call', entry name, [raw pointers]) in the same order, among which a RecordingHook
    puts its ('publish', tag, (lo, hi)) and ('finish',)."""

    def __init__(self):
        self.calls, self.events = [], []

    def clear(self):
        del self.calls[:], self.events[:]

    def _stream_step(self, name):
        def entry(stream, args):
            assert not stream, stream
            ptrs = []
            self.calls.append(_stream_form_call(name, args._obj, ptrs))
            self.events.append(('call', self.calls[-1][0], ptrs))
            return 0
        return entry

    def __getattr__(self, name):                                    # the fake library: any entry point
        if not name.startswith('tcow_'):
            raise AttributeError(name)
        if name in ('tcow_attn_temporal_step', 'tcow_cls_step'):
            return self._stream_step(name)
        declared = _lib.SIGNATURES[name][1]

        def entry(*args):
            assert len(args) == len(declared), (name, len(args), len(declared))
            ptrs = []
            self.calls.append([name] + [_argument(a, d, ptrs) for a, d in zip(args, declared)])
            self.events.append(('call', name, ptrs))
            return {'tcow_gemm_tn_group_max': 32, 'tcow_cast_desc_bytes': CAST_DESC_BYTES, 'tcow_adamw_chunk_bytes': ADAMW_CHUNK_BYTES,
                    'tcow_adamw_tile_bytes': ADAMW_TILE_BYTES}.get(name, 0)
        return entry


def install(monkeypatch):
    """The three replacements; returns the Trace that records from now on."""
    trace = Trace()
    monkeypatch.setattr(_lib, 'lib', lambda fmt='bf16': trace)
    monkeypatch.setattr(ops, '_stream', lambda: 0)
    monkeypatch.setattr(ops, '_need_cuda', lambda *ts: None)
    return trace


class RecordingHook:
    """A grad_hook that records what the backward publishes: the tag and the byte range of the flat bucket."""
    active = True

    def __init__(self, trace):
        self.trace = trace

    def __call__(self, tag, flat):
        self.trace.events.append(('publish', tag, (flat.data_ptr(), flat.data_ptr() + flat.numel() * flat.element_size())))

    def finish(self):
        self.trace.events.append(('finish',))


# ------------------------------------------------------------------------------------------------------------------------- the pinned cases

T, H, W, D, DEPTH, CLIPS = 4, 32, 48, 64, 3, 2                    # the smallest shapes at which every branch is still taken (S = 7 tokens per frame)


def make_net(precision, ca=1, attention_type='divided_space_time', norm_embeddings=False, depth=DEPTH):
    torch.manual_seed(0)
    net = Seeker(None, num_total_frames=T, frame_height=H, frame_width=W, network_depth=depth, embed_dim=D, num_heads=1, causal_attention=ca,
                 attention_type=attention_type, norm_embeddings=norm_embeddings, drop_path_rate=0.1, precision=precision)
    net.seeker._warned_ls = True                                  # (fp16 without an attached optimizer warns once; not the subject here)
    return net


def clip_inputs(queries=1, frames=T, clips=CLIPS):
    return torch.zeros(clips, 3, frames, H, W), torch.zeros(clips * queries, 1, frames, H, W)


def train_step(net, queries=1, flags_grad=True, hook=None, trace=None):
    """Forward + backward of one training step through SeekerFunction; trace (optional) is cleared between the two."""
    m = net.train().seeker
    if hook is not None:
        m.grad_hook, m.persistent_grads = hook, True
    rgb, qm = clip_inputs(queries)
    om, fl = engine.SeekerFunction.apply(m, rgb, qm, *m.param_list())
    if trace is not None:
        trace.clear()
    (om.sum() + fl.sum() if flags_grad else om.sum()).backward()
    return m


def eval_forward(net):
    m = net.eval().seeker
    with torch.no_grad():
        engine.run_forward(m, *clip_inputs(), m.param_list(), save=False)


def _forced(net):
    """Forced DropPath masks for some but not all (block, kind) keys."""
    N = (H // 16) * (W // 16)
    net.seeker.forced_drop_masks = {(0, 'temporal'): (torch.ones(CLIPS, N), 0.05), (1, 'spatial'): (torch.ones(CLIPS, T), 0.05),
                                    (1, 'mlp'): (torch.zeros(CLIPS), 0.05), (2, 'mlp'): (torch.ones(CLIPS), 0.1)}
    return net


def _resized(net):
    """Stored pos / time tables of another size than the clip's: 4 x 4 patches + cls instead of 2 x 3 + cls, 6 frames instead of 4."""
    v = net.seeker.vit
    v.pos_embed = torch.nn.Parameter(torch.zeros(1, 17, D))
    v.time_embed = torch.nn.Parameter(torch.zeros(1, 6, D))
    net.seeker.invalidate_param_cache()
    return net


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def stream_step(net, form, skinny):
    """One step of the given form, built directly on its state, through engine.run_forward."""
    m = net.eval().seeker
    with torch.no_grad():
        if form == 'paged':
            st = stream._PagedState(m, 2, skinny, 2, 4)
        else:
            st = stream._State(m, 2, skinny)
        if form in ('stream1', 'stream2'):
            c = int(form[-1])
            rows, frames, step = 2, c, stream._StreamStep(st, torch.empty(2 * c, D), torch.zeros(1, dtype=torch.int32))
        elif form == 'pool':
            rows, frames, step = 2, 1, stream._PoolStep(st, torch.empty(2, D), _i32([0, 2]), _i32([1, 0]))
        else:
            tab = stream.ragged_tables([0, 1], [0, 1], [1, 2])
            tables = [_i32(tab[k]) for k in ('t0', 'slot', 'first', 'c', 'row_of_frame')]
            if form == 'ragged':
                step = stream._RaggedStep(st, torch.empty(3, D), *tables)
            else:
                step = stream._PagedRaggedStep(st, torch.empty(3, D), *tables, _i32([[0, -1], [1, 2]]))
            rows, frames = 1, 3
        rgb, qm = clip_inputs(frames=frames, clips=rows)
        engine.run_forward(m, rgb, qm, m.param_list(), save=False, stream=step)


def _cases():
    c = {}
    for p in ('fp32', 'bf16', 'fp16', 'bf16x3'):
        c[f'train-{p}'] = lambda p=p: train_step(make_net(p))
        c[f'eval-{p}'] = lambda p=p: eval_forward(make_net(p))
    for p in ('bf16', 'fp32'):
        c[f'shared-rgb-{p}'] = lambda p=p: train_step(make_net(p), queries=2)
        c[f'joint-{p}'] = lambda p=p: train_step(make_net(p, ca=0, attention_type='joint_space_time'))
        c[f'norm-embeddings-{p}'] = lambda p=p: train_step(make_net(p, norm_embeddings=True))
        for form in ('stream1', 'stream2', 'pool', 'ragged', 'paged'):
            c[f'{form}-{p}'] = lambda p=p, form=form: stream_step(make_net(p), form, skinny=(p == 'bf16'))
    for ca in (0, 2, -1):
        c[f'causal{ca}-bf16'] = lambda ca=ca: train_step(make_net('bf16', ca=ca))
    c['forced-droppath-fp32'] = lambda: train_step(_forced(make_net('fp32')))
    c['resized-tables-fp32'] = lambda: train_step(_resized(make_net('fp32')))
    c['no-flags-gradient-bf16'] = lambda: train_step(make_net('bf16'), flags_grad=False)
    for spec in ('1', '2,1', '3'):
        c[f'group-{spec}-bf16'] = (lambda: train_step(make_net('bf16')), spec)
    return c


CASES = _cases()


def run_case(name, monkeypatch):
    """The normalised trace of a case, in the form the fixture stores (after a JSON round trip)."""
    case = CASES[name]
    if isinstance(case, tuple):
        case, spec = case
        monkeypatch.setenv('TCOW_DDP_GROUP', spec)
    else:
        monkeypatch.delenv('TCOW_DDP_GROUP', raising=False)
    trace = install(monkeypatch)
    torch.manual_seed(0)
    case()
    return json.loads(json.dumps(trace.calls))


def save_fixture(traces, path=FIXTURE):
    """{case: [call, ...]} as gzip'd JSON; a call that occurs many times is stored once (`calls`) and named by its index."""
    table, index = [], {}
    cases = {}
    for name, calls in traces.items():
        seq = []
        for call in calls:
            key = json.dumps(call)
            if key not in index:
                index[key] = len(table)
                table.append(call)
            seq.append(index[key])
        cases[name] = seq
    blob = json.dumps({'calls': table, 'cases': cases}, separators=(',', ':')).encode()
    with open(path, 'wb') as f:
        with gzip.GzipFile(fileobj=f, mode='wb', mtime=0) as z:
            z.write(blob)


def load_fixture(path=FIXTURE):
    with gzip.open(path, 'rb') as z:
        doc = json.loads(z.read().decode())
    return {name: [doc['calls'][i] for i in seq] for name, seq in doc['cases'].items()}
