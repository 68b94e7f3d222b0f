"""Host call-trace kit of FusedAdamWClip: every optimizer step on CPU tensors, without a device or the library -- which tables it hands to the
library, what is in them, every scalar, and the counters it keeps afterwards.

install(monkeypatch) builds on engine_trace.install (fake library, ops._stream = 0): it returns the fake library through a view that knows which
BUILD it stands for ('bf16' / 'fp16') and routes the optimizer's step entry point to a decoder.  A recorded step is normalised, so that it does
not depend on which entry point carried it:

  build                    the library build that was called
  chunks, flat, tiles      the decoded tables; every address is [parameter index, which of p / g / m / v / wc / wt, byte offset], resolved against
                           the tensors the optimizer is known to own (never by magnitude; an address outside all of them fails the run).  flat is
                           the chunk rows again when nothing is tiled, [] when everything is.
  lr ... max_norm, step    all scalars (floats as the f32 the library receives)
  scratch_len              elements of the scratch buffer (the pointer must be optimizer.scratch)
  inv_scale                whether an inverse loss scale was passed (the pointer must be the module's pending_inv_scale)

and the entry says whether the tables were 'rebuilt' or 'reused'.  Nothing computes: the scratch tail (coefficient, norm, skipped count) holds
what the case wrote into it by hand.  After every step the trace notes step_count, the per-parameter 'step' values, skipped_steps and
float(ls_log2).

CASES / run_case() are pinned by tests/golden/optim_calls.json.gz (tools/make_optim_calls.py writes it, from the commit BEFORE the optimizer's
entry points became one and its host arithmetic moved to tcow_amd/optim_plan.py; it is not regenerated to make a changed trace pass).

bits_run() is the GPU side: four real steps on fixed gradients, hashed (tools/make_optim_bits.py, tests/test_gpu_optim.py).
"""
import ctypes
import gzip
import hashlib
import json
import os

import numpy as np
import torch

import engine_trace
from tcow_amd import _lib
from tcow_amd._lib import TcowError
from tcow_amd.optim import FusedAdamWClip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURE = os.path.join(GOLDEN, 'optim_calls.json.gz')
BITS_FIXTURE = os.path.join(GOLDEN, 'optim_step_bits.json')
CHUNK_WORDS, TILE_WORDS = 5, 7                  # int64 words of a chunk record (40 bytes) and of a tile record (56 bytes)


def _f32(x):
    return ctypes.c_float(x).value


def _words(ptr, n):
    return list((ctypes.c_int64 * n).from_address(ptr)) if ptr and n else []


class Recorder:
    """Normalises the launches of one optimizer."""

    def __init__(self):
        self.opt, self.launches = None, []

    def _known(self):
        """[(first byte, last byte + 1, parameter index, which)] of every tensor a table may point into."""
        opt, out = self.opt, []
        reg = opt._tracker._operands.registry if opt._tracker is not None else {}
        for i, p in enumerate(opt.params):
            st = opt.state.get(p, {})
            ts = {'p': p, 'g': p.grad, 'm': st.get('exp_avg'), 'v': st.get('exp_avg_sq')}
            if id(p) in reg:
                ts['wc'], ts['wt'] = reg[id(p)][1], reg[id(p)][2]
            out += [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), i, w) for w, t in ts.items() if t is not None]
        return out

    def _address(self, a, known):
        hits = [[i, w, a - lo] for lo, hi, i, w in known if lo <= a < hi]
        assert len(hits) == 1, ('address in none or several of the known tensors', hex(a), hits)
        return hits[0]

    def launch(self, build, chunks, n_chunks, flat, n_flat, tiles, n_tiles, floats, step, max_norm, scratch, inv_scale):
        """The arguments of a step in the terms of tcow_adamw_args; floats = (lr, beta1, beta2, eps, weight_decay)."""
        opt, known = self.opt, self._known()
        rows = lambda ptr, n: [[self._address(a, known) for a in r[:4]] + [r[4]] for r in np.reshape(_words(ptr, n * CHUNK_WORDS), (-1, CHUNK_WORDS)).tolist()]
        recs = [[self._address(a, known) for a in r[:6]] + [r[6] & 0xffffffff, r[6] >> 32]           # CastTile: ... int K, N
                for r in np.reshape(_words(tiles, n_tiles * TILE_WORDS), (-1, TILE_WORDS)).tolist()]
        assert scratch == opt.scratch.data_ptr()
        inv = opt._tracker.pending_inv_scale if opt._tracker is not None else None
        assert (inv_scale or None) == (None if inv is None else inv.data_ptr())
        names = ('lr', 'beta1', 'beta2', 'eps', 'weight_decay')
        self.launches.append(dict({k: _f32(v) for k, v in zip(names, floats)}, build=build, chunks=rows(chunks, n_chunks), flat=rows(flat, n_flat), tiles=recs,
                                  step=int(step), max_norm=_f32(max_norm), scratch_len=opt.scratch.numel(), inv_scale=bool(inv_scale)))


def step_entries(rec):
    """{entry name: f(build, *arguments)} for the library's optimizer step."""
    def clip_step(build, stream, args):
        a = args._obj
        rec.launch(build, a.chunks, a.n_chunks, a.flat_chunks, a.n_flat, a.tiles, a.n_tiles, (a.lr, a.beta1, a.beta2, a.eps, a.weight_decay), a.step, a.max_norm,
                   a.scratch, a.grad_inv_scale)
        return 0
    return {'tcow_adamw_clip_step': clip_step}


class _Build:
    """The fake library as one build of it."""

    def __init__(self, trace, build, entries):
        self._trace, self._build, self._entries = trace, build, entries

    def __getattr__(self, name):
        if name in self._entries:
            return lambda *args: self._entries[name](self._build, *args)
        return getattr(self._trace, name)


def install(monkeypatch, entries=step_entries):
    """engine_trace's replacements, with the optimizer's step routed to a Recorder; returns the Recorder."""
    trace, rec = engine_trace.install(monkeypatch), Recorder()
    table = entries(rec)
    builds = {b: _Build(trace, b, table) for b in ('bf16', 'fp16')}
    monkeypatch.setattr(_lib, 'lib', lambda fmt='bf16': builds[fmt])
    return rec


class Driver:
    """Runs steps of one optimizer and appends to the trace what each launched and the counters after it."""

    def __init__(self, rec, trace, make):
        self.rec, self.trace = rec, trace
        try:
            self.opt = rec.opt = make()
        except TcowError as e:
            self.opt = None
            trace.append(['refused', str(e)])
        self.kept = []                                              # replaced tensors, so that no new one gets an old one's address

    def counters(self):
        opt = self.opt
        ls = getattr(opt._tracker, 'ls_log2', None) if opt._tracker is not None else None
        skipped = opt.skipped_steps
        return {'step_count': opt.step_count, 'steps': [float(opt.state[p]['step']) if 'step' in opt.state.get(p, {}) else None for p in opt.params],
                'skipped_steps': None if skipped is None else float(skipped), 'ls_log2': None if ls is None else float(ls)}

    def step(self):
        opt, rec = self.opt, self.rec
        table = opt._table
        del rec.launches[:]
        try:
            opt.step()
        except TcowError as e:
            self.trace.append(['refused', str(e)])
            return
        assert len(rec.launches) <= 1
        self.kept.append(table)
        tables = None if not rec.launches else 'reused' if opt._table is table else 'rebuilt'
        self.trace.append(['step', {'tables': tables, 'launch': rec.launches[0] if rec.launches else None}])
        self.trace.append(['counters', self.counters()])

    def give_grads(self, indices, value=1.0):
        """New gradient tensors for these parameters (the ones they had stay alive)."""
        for i in indices:
            p = self.opt.params[i]
            self.kept.append(p.grad)
            p.grad = torch.full_like(p, value)

    def note(self, what, value):
        self.trace.append([what, value])


# ------------------------------------------------------------------------------------------------------------------------- the pinned cases

SIZES = [(1,), (3,), (4,), (7,), (65536,), (65537,), (3, 5), (2,)]          # one vector plus a tail ... two chunks, the second of one element; 2-D; never a gradient
NO_GRAD = len(SIZES) - 1


def plain_params():
    return [torch.nn.Parameter(torch.zeros(s)) for s in SIZES]


def plain_optimizer(rec, tr, **kw):
    d = Driver(rec, tr, lambda: FusedAdamWClip(plain_params(), lr=1e-3, max_norm=0.3, **kw))
    d.give_grads(range(NO_GRAD))
    return d


def case_three_steps(rec, tr):
    d = plain_optimizer(rec, tr)
    for _ in range(3):                                              # build, then the fast path twice
        d.step()


def case_grad_replaced(rec, tr):
    d = plain_optimizer(rec, tr)
    d.step()
    d.opt.scratch[-1] = 1.0                                         # one step skipped so far: carried into the new scratch buffer
    d.give_grads([2])
    d.step(); d.step()
    d.give_grads([0, 6])                                            # the first one: the address test of the fast path
    d.step()


def case_grad_none(rec, tr):
    d = plain_optimizer(rec, tr)
    d.step()
    d.opt.params[3].grad = None
    d.step(); d.step()
    for p in d.opt.params:
        p.grad = None
    d.step()                                                        # nothing to do


def case_load_state_dict(rec, tr):
    d = plain_optimizer(rec, tr)
    d.step(); d.step()
    d.opt.scratch[-1] = 1.0
    sd = d.opt.state_dict()
    d.note('saved steps', [float(st['step']) for st in sd['state'].values()])
    d.opt.load_state_dict(sd)
    d.note('skipped after load', d.opt.skipped_steps)
    d.step(); d.step()


def case_late_gradient(rec, tr):
    d = plain_optimizer(rec, tr)
    first, late = d.opt.params[0], d.opt.params[4]
    d.kept += [first.grad, late.grad]
    first.grad = late.grad = None
    d.step(); d.step()
    d.give_grads([4])                                               # thawed after the others have stepped twice: everybody goes on with step 3
    d.step()
    d.give_grads([0])                                               # and one that comes first in the table
    d.step(); d.step()


def case_state_dict_with_skips(rec, tr):
    d = plain_optimizer(rec, tr)
    for _ in range(3):
        d.step()
    d.opt.scratch[-1] = 2.0
    sd = d.opt.state_dict()
    d.note('saved steps', [float(st['step']) for st in sd['state'].values()])
    d.note('saved groups', [[k, v] for k, v in sorted(sd['param_groups'][0].items()) if k in ('lr', 'betas', 'eps', 'weight_decay', 'params')])
    d.note('live steps', [float(d.opt.state[p]['step']) if p in d.opt.state else None for p in d.opt.params])
    d.step()
    d.opt.param_groups[0]['lr'] = 3e-4                             # what a scheduler does: read every step
    d.opt.max_norm = None
    d.step()


def case_refusals(rec, tr):
    a, b = plain_params()[:2]
    Driver(rec, tr, lambda: FusedAdamWClip([{'params': [a]}, {'params': [b]}]))
    for p in (torch.nn.Parameter(torch.zeros(4, 6).t()), torch.nn.Parameter(torch.zeros(5, dtype=torch.float64))):
        d = Driver(rec, tr, lambda: FusedAdamWClip([torch.nn.Parameter(torch.zeros(3)), p]))
        d.give_grads([0])
        d.opt.params[1].grad = torch.ones_like(p)                   # (full_like would come out contiguous)
        d.step()


def module_optimizer(rec, tr, precision, **kw):
    """The trace kit's net with persistent gradient buckets and an optimizer attached; a training forward + backward has run."""
    net = engine_trace.make_net(precision)
    net.seeker.persistent_grads = True
    d = Driver(rec, tr, lambda: FusedAdamWClip(list(net.parameters()), lr=1e-3, max_norm=0.3, module=net, **kw))
    d.net, d.m = net, net.seeker
    d.backward = lambda: engine_trace.train_step(net)
    d.backward()
    return d


def case_module(rec, tr, precision, fuse):
    d = module_optimizer(rec, tr, precision, fuse_cast=fuse)
    d.step()
    d.backward(); d.step()                                          # the same buckets, the same operand copies: the fast path
    d.step()
    d.m._operands.drop(buckets=False)                               # the generation moved (and nothing is registered: every parameter is updated flat)
    d.step()
    d.backward(); d.step()                                          # registered again
    d.m._operands.drop()                                            # the gradient buckets went too
    d.backward(); d.step(); d.step()


def case_fp16_scale(rec, tr):
    d = module_optimizer(rec, tr, 'fp16')
    d.note('pending_inv_scale', d.m.pending_inv_scale is not None)
    d.step()                                                        # inverse scale passed; coefficient 0: the exponent would creep, capped at -2
    d.m.pending_inv_scale = None
    d.step()                                                        # none passed
    d.backward()
    d.opt.scratch[-3] = -1.0                                        # what a skipped step leaves: the exponent drops by 4
    d.step()
    d.opt.scratch[-3] = 0.0
    d.step(); d.step()                                              # creeps back by 1 / 256 a step
    d.m.loss_scale = 1024.0                                         # static: no feedback
    d.opt.scratch[-3] = -1.0
    d.step()


def case_unscale_detach(rec, tr, precision):
    d = module_optimizer(rec, tr, precision)
    g = d.opt.params[0].grad
    g.fill_(3.0)                                                    # (nothing computes: the backward left it uninitialised)
    before = g.clone()
    inv = d.m.pending_inv_scale
    d.note('pending_inv_scale', inv is not None)
    d.opt.unscale_()
    d.note('after unscale_', [d.m.pending_inv_scale is None, bool(torch.equal(g, before * (1.0 if inv is None else inv)))])
    d.step()
    d.backward()
    d.opt.detach()
    d.note('after detach', [d.m.pending_inv_scale is None, d.m._live_optim() is None])
    d.backward()
    d.note('pending_inv_scale', d.m.pending_inv_scale is not None)
    d.step()


def _cases():
    c = {'three-steps': case_three_steps, 'grad-replaced': case_grad_replaced, 'grad-none': case_grad_none, 'load-state-dict': case_load_state_dict,
         'late-gradient': case_late_gradient, 'state-dict-with-skips': case_state_dict_with_skips, 'refusals': case_refusals,
         'fp16-scale': case_fp16_scale}
    for p in ('bf16', 'fp16', 'fp32'):
        for fuse in (True, False):
            c[f"module-{p}-{'fuse' if fuse else 'nofuse'}"] = lambda rec, tr, p=p, fuse=fuse: case_module(rec, tr, p, fuse)
    for p in ('fp16', 'bf16'):
        c[f'unscale-detach-{p}'] = lambda rec, tr, p=p: case_unscale_detach(rec, tr, p)
    return c


CASES = _cases()


def run_case(name, monkeypatch, entries=step_entries):
    """The trace of a case, in the form the fixture stores (after a JSON round trip)."""
    rec, trace = install(monkeypatch, entries), []
    torch.manual_seed(0)
    CASES[name](rec, trace)
    return json.loads(json.dumps(trace))


def save_fixture(traces, path=FIXTURE):
    blob = json.dumps(traces, separators=(',', ':'), sort_keys=True).encode()
    with open(path, 'wb') as f:
        with gzip.GzipFile(fileobj=f, mode='wb', mtime=0) as z:
            z.write(blob)


def load_fixture(path=FIXTURE):
    with gzip.open(path, 'rb') as z:
        return json.loads(z.read().decode())


# ------------------------------------------------------------------------------------------------------------------------- GPU: bits of four steps

BITS_EXTRAS = [(1,), (3,), (7,), (65537,), (5,)]                    # free parameters beside the net's; the last never gets a gradient


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def bits_run(precision, device='cuda:0'):
    """Four steps of FusedAdamWClip(module=net) on fixed gradients -- clipped; loss-scaled by 2^7 and unclipped; one inf: skipped; a normal one, whose
    bias correction runs with step - skipped -- on a depth-1 net of the trace kit's geometry plus BITS_EXTRAS.  Per step: sha256 of every parameter,
    both moments and the registered plain weights' operand copies, and the exact grad_norm, skipped_steps and ls_log2."""
    net = engine_trace.make_net(precision, depth=1).to(device).train()
    m = net.seeker
    m.persistent_grads = True
    net(*(t.to(device) for t in engine_trace.clip_inputs()))        # one training-mode forward registers the operand copies
    extras = [torch.nn.Parameter(torch.from_numpy(np.random.default_rng(100 + i).standard_normal(s).astype(np.float32)).to(device)) for i, s in enumerate(BITS_EXTRAS)]
    params = list(net.parameters()) + extras
    opt = FusedAdamWClip(params, lr=1e-3, max_norm=0.3, module=net)
    live = params[:-1]
    for p in live:
        p.grad = torch.zeros_like(p)

    def fill(seed, scale):
        rng = np.random.default_rng(seed)
        for p in live:
            p.grad.copy_(torch.from_numpy((rng.standard_normal(tuple(p.shape)) * scale).astype(np.float32)))

    out = []
    for k in range(4):
        if k == 0:
            fill(1, 10.0)
        elif k == 1:
            fill(2, 1e-5 * 2.0 ** 7)
            m.pending_inv_scale = torch.tensor(2.0 ** -7, dtype=torch.float32, device=device)
        elif k == 2:
            m.pending_inv_scale = None
            fill(3, 1e-3)
            live[3].grad.view(-1)[0] = float('inf')
        else:
            fill(4, 1e-3)
        opt.step()
        torch.cuda.synchronize()
        reg = m._operands.registry
        copies = [[_sha(reg[id(p)][1]) if reg[id(p)][1] is not None else None, _sha(reg[id(p)][2])] for p in params if id(p) in reg]
        out.append({'params': [_sha(p) for p in params],
                    'exp_avg': [_sha(opt.state[p]['exp_avg']) for p in live], 'exp_avg_sq': [_sha(opt.state[p]['exp_avg_sq']) for p in live],
                    'copies': copies, 'grad_norm': float(opt.grad_norm()).hex(), 'skipped_steps': float(opt.skipped_steps).hex(),
                    'ls_log2': float(m.ls_log2).hex(), 'tiles': 0 if opt._tiles is None else int(opt._tiles.shape[0])})
    return out
