"""Fused clip_grad_norm_ + AdamW for the Seeker training step (train.py:99-102, 239-243) on libtcow_hip.

Same arithmetic as torch.nn.utils.clip_grad_norm_(params, max_norm) followed by torch.optim.AdamW(params, lr).step()
(betas (0.9, 0.999), eps 1e-8, weight_decay 0.01 on every parameter -- the reference builds one parameter group with torch's
defaults), but as three kernel launches over a device-resident chunk table instead of ~250 per-tensor
foreach operations.  Parameters without a gradient are skipped, like torch does.

It IS a torch.optim.Optimizer: `param_groups` carries lr / betas / eps / weight_decay (read every step, so the reference's
MultiStepLR, train.py:236-243, attaches unchanged), and `state_dict()` / `load_state_dict()` use torch.optim.AdamW's layout
(per-parameter 'step', 'exp_avg', 'exp_avg_sq'), so a reference checkpoint's 'optim_seeker' (train.py:282) loads and what is
saved here loads into torch.optim.AdamW.

The kernels write the parameters through raw pointers; after every step the parameters' autograd version counters are bumped
(torch.autograd.graph.increment_version), so anything that caches derived copies keyed on `p._version` -- the Seeker's bf16
operand copies are -- can never serve stale weights.  `on_step` callbacks (e.g. QueryMaskTracker.invalidate_weight_cache, which
re-casts all GEMM operands in ONE launch) are an optimisation on top of that, not a correctness requirement.

One extension over torch's pair: a step whose total gradient norm is NaN / infinite is SKIPPED (parameters and moments untouched) instead
of poisoning the weights -- the overflow guard of the binary16 mode (precision='fp16'), whose loss-scale exponent is lowered in the same
step (device side, no synchronisation).  Skips are COUNTED on the device in every precision (`skipped_steps`, a device scalar; read it
-- one sync -- whenever you log: a NaN gradient in bf16 / fp32 training shows up there instead of silently freezing the weights), and the
update kernel subtracts them from the step number of its bias correction, so moments and correction stay in step; `state_dict()`
stores the applied-update count, i.e. what torch.optim.AdamW would have counted behind a GradScaler.  The arithmetic of the
pointer tables is optim_plan.py's."""
import ctypes
import weakref

import numpy as np
import torch

from . import _lib as L
from . import ops
from . import optim_plan as plan


class FusedAdamWClip(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_norm=0.3, module=None, fuse_cast=True):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if len(self.param_groups) != 1:
            raise L.TcowError('FusedAdamWClip takes one parameter group (train.py:239-241 builds exactly one)')
        self.max_norm = max_norm
        self.scratch = None        # f32 [chunks + 3]: the chunks' partial sums | clip coefficient, gradient norm, skipped steps
        self.on_step = []          # callables run after every step
        self._tracker = None
        self._skip_carry = 0.0         # skipped steps of earlier pointer tables (the device counter lives in the scratch buffer)
        self._live = []; self._seen_grads = []; self._step_base = 0; self._steps_pending = 0
        # fuse_cast (16-bit modes, module= given): GEMM weights are updated tile by tile and the update writes their 16-bit W / W^T operand copies itself
        # -- the module's batched re-cast then only covers what is left (the folded products)
        self.fuse_cast = bool(fuse_cast)
        # made by _build(): chunks of every live parameter | the flat-updated ones (the same tensor when nothing is tiled) | tiles or None, and what they were built for
        self._table = self._flat_table = self._tiles = None; self._cast_keys = frozenset(); self._key = None; self._operand_gen = None
        if module is not None:     # a Seeker / QueryMaskTracker: batch re-cast of its GEMM operand copies right after the update
            tracker = self._tracker = getattr(module, 'seeker', module)
            if hasattr(tracker, 'invalidate_weight_cache'):
                self.on_step.append(tracker.invalidate_weight_cache)
            # A WEAK reference to the attached optimizer (QueryMaskTracker._live_optim).  While it is alive, precision='fp16' has somebody who lowers the loss scale
            # after an overflow (run_backward warns otherwise), and -- with persistent_grads, one backward per step -- gradient buckets may stay loss-scaled:
            # step() folds the inverse scale into the clip coefficient.  Once this optimizer is discarded the module unscales in the backward again.
            tracker._optim_ref = weakref.ref(self)
        if (L.lib().tcow_adamw_chunk_bytes(), L.lib().tcow_adamw_tile_bytes()) != (plan.CHUNK_BYTES, plan.TILE_BYTES):
            raise L.TcowError('the chunk / tile records of the library are not the ones optim_plan.py writes')

    @property
    def params(self):
        return self.param_groups[0]['params']

    @property
    def lr(self):
        return self.param_groups[0]['lr']

    @property
    def step_count(self):
        self._flush_steps()
        for p in self.params:
            st = self.state.get(p)
            if st:
                return int(st['step'])
        return 0

    def _flush_steps(self):
        """state[p]['step'] (CPU scalars, torch.optim.AdamW's layout) += the steps taken since the last flush: one foreach call when the state is
        read (state_dict, step_count, table rebuild) instead of one per step."""
        if self._steps_pending and self._live:
            torch._foreach_add_([self.state[p]['step'] for p in self._live], float(self._steps_pending))
            self._step_base += self._steps_pending
        self._steps_pending = 0

    def _build(self, live):
        """Tables, scratch buffer and argument structure for these parameters, in this order (the partial sums of the norm are folded in it)."""
        trk, dev = self._tracker, live[0].device
        own = self.fuse_cast and trk is not None and getattr(trk, 'precision', None) in ('bf16', 'fp16') and not getattr(trk, '_is_replica', False)
        reg = trk._operands.castable() if own else {}      # {id(parameter): (Wc, Wt, N, K)} of the GEMM weights whose 16-bit operand copies this optimizer may write (the module's registry of the current training forward)
        quads = []
        for p in live:
            st = self.state[p]
            if 'exp_avg' not in st:
                st['step'] = torch.tensor(0.0, dtype=torch.float32)
                st['exp_avg'], st['exp_avg_sq'] = (torch.zeros_like(p, dtype=torch.float32, memory_format=torch.preserve_format) for _ in range(2))
            quad = (p, p.grad, st['exp_avg'], st['exp_avg_sq'])
            if not all(t.is_contiguous() and t.dtype == torch.float32 for t in quad):
                raise L.TcowError('FusedAdamWClip needs contiguous f32 parameters, gradients and moments')
            quads.append(tuple(t.data_ptr() for t in quad))
        tiled = [i for i, p in enumerate(live) if id(p) in reg]
        rows, owner = plan.chunk_rows([q + (p.numel(),) for q, p in zip(quads, live)])
        if self.scratch is not None:
            self._skip_carry += float(self.scratch[-1])      # (rebuilds are rare: first step, re-allocated gradients, load_state_dict)
        self.scratch = torch.zeros(len(rows) + 3, dtype=torch.float32, device=dev)
        self.scratch[-1] = self._skip_carry
        flat = self._table = self._flat_table = torch.from_numpy(rows).to(dev)
        tiles = self._tiles = None
        if tiled:
            recs = [plan.tile_records(*quads[i], Wc.data_ptr(), Wt.data_ptr(), N, K) for i in tiled for Wc, Wt, N, K in (reg[id(live[i])],)]
            tiles = self._tiles = torch.from_numpy(np.concatenate(recs, axis=0)).to(dev)
            flat = self._flat_table = torch.from_numpy(plan.flat_rows(rows, owner, tiled)).to(dev)
        self._cast_keys, self._operand_gen = frozenset(id(live[i]) for i in tiled), trk._operands.generation if trk is not None else None
        self._lib = L.lib('fp16') if tiled and trk.precision == 'fp16' else L.lib()      # the build whose 16-bit format the operand copies have; nothing tiled, nothing 16-bit is written: the bf16 build serves
        self._args = L.AdamwArgs(chunks=self._table.data_ptr(), n_chunks=len(rows), flat_chunks=flat.data_ptr() if len(flat) else None, n_flat=len(flat),
                                 tiles=tiles.data_ptr() if tiled else None, n_tiles=len(tiles) if tiled else 0, scratch=self.scratch.data_ptr())
        self._args_ref = ctypes.byref(self._args)          # (lr ... grad_inv_scale: _launch, every step)

    def _tables(self, params):
        """Step 1: the tables of this step's live parameters, reused or rebuilt.  False: no parameter has a gradient."""
        # Fast path (every step but the first): the same Parameter list with the same gradient TENSOR OBJECTS as when the pointer table was
        # built (persistent gradient buckets), first / last gradient still at the recorded address -- one identity test per parameter instead of
        # two data_ptr() calls and a Tensor.__hash__ dictionary lookup each (0.7 ms of host time per step over ~250 parameters).
        fast, trk = self._key is not None and len(params) == len(self._seen_grads), self._tracker
        if fast:
            for p, g in zip(params, self._seen_grads):
                if p.grad is not g:
                    fast = False
                    break
        fast = fast and self._live[0].grad.data_ptr() == self._key[0][1] and self._live[-1].grad.data_ptr() == self._key[-1][1]      # (a key is never kept without its live parameters)
        if fast and (trk is None or not self.fuse_cast or trk._operands.generation == self._operand_gen):
            return True
        live = [p for p in params if p.grad is not None]
        if not live:
            return False
        self._flush_steps()
        key = lambda: plan.table_key([id(p) for p in live], [p.grad.data_ptr() for p in live], [self.state[p]['exp_avg'].data_ptr() if 'exp_avg' in self.state[p] else 0 for p in live])
        if not plan.tables_current(key(), trk._operands.generation if trk is not None else None, self._key, self._operand_gen, self.fuse_cast):
            self._build(live)
            self._key = key()
        self._live, self._seen_grads = live, [p.grad for p in params]
        self._step_base, self._steps_pending = plan.step_base(int(self.state[p]['step']) for p in live), 0
        return True

    def _launch(self):
        """Step 2: the per-step arguments and the call."""
        grp, a, trk = self.param_groups[0], self._args, self._tracker
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = float(grp['lr']), float(grp['betas'][0]), float(grp['betas'][1]), float(grp['eps']), float(grp['weight_decay'])
        a.step, a.max_norm = self._step_base + self._steps_pending + 1, float(self.max_norm or 0.0)
        inv_scale = trk.pending_inv_scale if trk is not None else None      # binary16: the last backward left its gradients loss-scaled (it stays valid until the next backward rewrites them)
        a.grad_inv_scale = inv_scale.data_ptr() if inv_scale is not None else None
        L.check(self._lib.tcow_adamw_clip_step(ops._stream(), self._args_ref), 'tcow_adamw_clip_step', self._lib)
        if self._tiles is not None:
            trk._operands.optimizer_wrote(self._cast_keys)          # (consumed by the module's OperandCache.refresh in the on_step callback)

    def _loss_scale_feedback(self):
        """Step 3, precision='fp16': a non-finite gradient norm means the scaled backward overflowed binary16 -- the kernels skipped the update
        (clip coefficient -1); lower the module's loss-scale exponent by 4, otherwise let it creep back towards -2.  All on the device."""
        trk = self._tracker
        ls = getattr(trk, 'ls_log2', None) if trk is not None and getattr(trk, 'precision', None) == 'fp16' and getattr(trk, 'loss_scale', None) == 'dynamic' else None
        if ls is not None and ls.device == self.scratch.device:
            ok = self.scratch[-3] >= 0                       # clip coefficient -1 = skipped
            ls.copy_(torch.minimum(ls + torch.where(ok, 1.0 / 256.0, -4.0), torch.full_like(ls, -2.0)))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not self._tables(self.param_groups[0]['params']):
            return loss
        self._launch()
        self._loss_scale_feedback()
        self._steps_pending += 1    # the per-parameter 'step' scalars of torch.optim.AdamW's state layout are brought up to date when somebody looks (_flush_steps)
        torch.autograd.graph.increment_version(self._live)   # the kernels wrote through raw pointers: make the update visible to version checks
        for cb in self.on_step:
            cb()
        return loss

    def unscale_(self):
        """precision='fp16' with persistent_grads: param.grad holds LOSS-SCALED gradients between backward and step() (torch.cuda.amp.GradScaler's
        convention; step() undoes the scale on the fly).  Call this first when something else must see true gradients in between -- clip_grad_norm_,
        gradient logging, another optimizer: multiplies every live gradient by the pending inverse scale (one pass over the gradients) and clears it.
        A no-op in every other mode."""
        trk = self._tracker
        inv = trk.pending_inv_scale if trk is not None else None
        if inv is None:
            return
        seen = set()
        for p in self.params:
            if p.grad is not None and p.grad.data_ptr() not in seen:
                seen.add(p.grad.data_ptr())
                p.grad.mul_(inv)
        trk.pending_inv_scale = None

    def detach(self):
        """Detach from the module given as module= (its fp16 backwards unscale their gradients themselves again)."""
        trk = self._tracker
        if trk is not None:
            self.unscale_()
            if trk._live_optim() is self:
                trk._optim_ref = None

    def grad_norm(self):
        """Total gradient norm of the last step (device tensor, no sync)."""
        return self.scratch[-2]

    @property
    def skipped_steps(self):
        """Steps skipped so far because their gradient norm was not finite (device f32 scalar, no sync; None before the first step)."""
        return None if self.scratch is None else self.scratch[-1]

    def state_dict(self):
        """torch.optim.AdamW's layout; 'step' = updates actually applied (calls minus skipped steps; one device read here, none per step)."""
        self._flush_steps()
        sd = super().state_dict()
        skipped = float(self.scratch[-1]) if self.scratch is not None else 0.0
        if skipped:
            # torch's Optimizer.state_dict() hands out the LIVE per-parameter dicts: adjust copies, never self.state (the device counter is
            # subtracted again inside the update kernel, so rewriting the live 'step' would double-count every skip after each save)
            sd['state'] = {k: dict(st) for k, st in sd['state'].items()}
            for st in sd['state'].values():
                if 'step' in st:
                    st['step'] = st['step'] - skipped
        return sd

    def load_state_dict(self, sd):
        self._steps_pending = 0           # (the loaded counters replace whatever was pending)
        super().load_state_dict(sd)
        self._key = None; self._live = []; self._seen_grads = []
        self._skip_carry = 0.0            # the loaded 'step' already counts applied updates only
        self.scratch = None
