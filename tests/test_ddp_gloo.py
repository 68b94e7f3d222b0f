"""CPU, world_size 2 over gloo: the bucketed gradient averaging used by the data-parallel step."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from tcow_amd import ddp, synth
    r, lr, w = ddp.init_distributed(backend='gloo')
    assert (r, w) == (rank, world)
    sync = ddp.GradSync(world)
    buckets = {name: torch.full((n,), float(rank + 1) * (i + 1)) for i, (name, n) in enumerate([('head', 7), (1, 1000), (0, 1000), ('embed', 33)])}
    for name, flat in buckets.items():
        sync(name, flat)                       # engine.run_backward fires the hook in exactly this way, bucket by bucket
    sync.finish()
    ok = all(torch.allclose(flat, torch.full_like(flat, 1.5 * (i + 1))) for i, flat in enumerate(buckets.values()))
    late = ddp.GradSync(world, overlap=False)          # the non-overlapped fallback: nothing is sent before finish()
    b2 = {name: torch.full((n,), float(rank + 1) * (i + 1)) for i, (name, n) in enumerate([('head', 5), (0, 64)])}
    for name, flat in b2.items():
        late(name, flat)
    ok = ok and len(late.pending) == 0 and all(torch.equal(flat, torch.full_like(flat, float(rank + 1) * (i + 1))) for i, flat in enumerate(b2.values()))
    late.finish()
    ok = ok and all(torch.allclose(flat, torch.full_like(flat, 1.5 * (i + 1))) for i, flat in enumerate(b2.values()))
    half = ddp.GradSync(world, bucket_dtype='bf16')    # bf16 on the wire, f32 bucket in and out
    b3 = torch.full((300,), float(rank + 1) * 0.25)
    half('blk', b3); half.finish()
    ok = ok and b3.dtype == torch.float32 and torch.equal(b3, torch.full_like(b3, 0.375)) and half.bytes == 300 * 2
    lin = torch.nn.Linear(4, 4)
    torch.manual_seed(rank); torch.nn.init.normal_(lin.weight)
    ddp.broadcast_parameters(lin)
    gathered = [torch.zeros_like(lin.weight) for _ in range(world)]
    dist.all_gather(gathered, lin.weight.data)
    ok = ok and torch.equal(gathered[0], gathered[1])
    clip_a = synth.make_clip(1, 2, 16, 16, seed=ddp.shard_seed(900, rank))['rgb']
    ok = ok and sync.launched == ['head', 1, 0, 'embed'] and sync.bytes == (7 + 2000 + 33) * 4
    st = sync.stats()                              # the fields bench.py puts into its N > 1 line
    ok = ok and st['buckets'] == 4 and st['allreduce_bytes'] == (7 + 2000 + 33) * 4 and st['allreduce_exposed_ms'] >= 0.0 and st['bucket_dtype'] == 'f32' 
    q.put((rank, bool(ok), float(clip_a.sum())))
    dist.destroy_process_group()


def test_gradsync_two_ranks_gloo():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs: p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs: p.join(timeout=60)
    assert all(ok for _, ok, _ in res)
    assert res[0][2] != res[1][2]              # ranks draw different clips (weak scaling: 1 clip per rank)


def test_single_process_is_a_noop():
    from tcow_amd import ddp
    sync = ddp.GradSync(1)
    t = torch.ones(5)
    sync('x', t); sync.finish()
    assert torch.equal(t, torch.ones(5)) and sync.pending == []


def test_a_hook_of_one_rank_says_it_is_inactive():
    """engine.run_backward leaves the binary16 loss scale to the optimizer only when no ACTIVE data-parallel hook is attached (ranks choose their own
    scales, so buckets must be unscaled before they are averaged): a GradSync of one rank is inactive unless forced."""
    from tcow_amd import ddp
    assert ddp.GradSync(world_size=1).active is False
    assert ddp.GradSync(world_size=1, force=True).active is True
    assert ddp.GradSync(world_size=2).active is True


def test_bench_self_launches_n_ranks():
    """`python bench.py --gpus 2` with no launcher around it must start two ranks itself (it silently ran one) --
    exercised on CPU through the launch self-test (gloo), which stops before any GPU work."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ); env.pop('WORLD_SIZE', None); env.pop('RANK', None); env['TCOW_DIST_BACKEND'] = 'gloo'
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--launch-selftest'], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith('{')][-1]
    res = json.loads(line)
    assert res['n_gpus'] == 2 and res['ranks_seen'] == 2
    # a rank count that does not match --gpus is an error, not a silent single-GPU run
    env2 = dict(env, WORLD_SIZE='1', RANK='0')
    bad = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1'], env=env2, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and 'WORLD_SIZE' in (bad.stderr + bad.stdout)


def test_a_failing_rank_surfaces_in_rank_zeros_line_instead_of_a_hang():
    """a rank != 0 that raises after the rendezvous (here rank 1, injected) while rank 0 already sits in the next collective.  The run must
    end within seconds -- not at the collective timeout --, with ONE JSON line on stdout whose `ddp.error` names the rank and the exception, and a
    non-zero exit code.  Rank 0 failing itself gives the same line."""
    import json
    import subprocess
    import sys
    import time
    from conftest import ROOT
    for bad_rank in (1, 0):
        env = dict(os.environ); env.pop('WORLD_SIZE', None); env.pop('RANK', None)
        env.update(TCOW_DIST_BACKEND='gloo', TCOW_BENCH_FAIL_RANK=str(bad_rank), TCOW_DIST_TIMEOUT_S='600')
        t0 = time.time()
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--launch-selftest'], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode != 0 and time.time() - t0 < 120, (out.returncode, out.stderr[-1500:])
        lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
        assert len(lines) == 1, out.stdout[-1500:]
        res = json.loads(lines[0])
        assert res['value'] is None and res['n_gpus'] == 2
        err = res['ddp']['error']
        assert [e['rank'] for e in err] == [bad_rank] and err[0]['type'] == 'RuntimeError' and 'injected failure' in err[0]['message']


def test_first_contact_and_bucket_timeline_fields():
    """ddp.first_contact outside a process group is a no-op record; GradSync.stats() carries the per-bucket timeline key (None on the CPU path)."""
    from tcow_amd import ddp
    c = ddp.first_contact()
    assert c['world'] == 1 and c['ms'] == 0.0
    st = ddp.GradSync(1).stats()
    assert 'bucket_timeline' in st and st['bucket_timeline'] is None
    assert ddp.rccl_version() is None or isinstance(ddp.rccl_version(), str)


def test_group_sizes_spec():
    """TCOW_DDP_GROUP: one number or a comma list, top group first; the bottom group is small by default (its all-reduce cannot overlap)."""
    from tcow_amd.engine import group_sizes
    assert group_sizes(12, '4') == [4, 4, 4] and group_sizes(12, '5') == [5, 5, 2] and group_sizes(12, '5,5,2') == [5, 5, 2]
    assert group_sizes(12, '6,3') == [6, 3, 3] and group_sizes(4, '2') == [2, 2] and group_sizes(3, '8') == [3] and group_sizes(12, '12') == [12]
    assert sum(group_sizes(24, None if 'TCOW_DDP_GROUP' not in os.environ else '4')) == 24
    assert group_sizes(12, '5,5,2') == group_sizes(12, None) or 'TCOW_DDP_GROUP' in os.environ


def _bucket_tags(depth, spec, fold):
    """The tags engine.run_backward publishes, in order: 'g<lowest block>' of every group above the bottom one from the top down, the late
    fold bucket, the bottom group."""
    from tcow_amd.engine import group_sizes
    tags, hi = [], depth
    for gs in group_sizes(depth, spec):
        hi -= gs
        if hi > 0:
            tags.append('g%d' % hi)
    return tags + (['fold'] if fold else []) + ['g0']


# gradients that torch ops write (a copy_ of a reduced table), not a library call; model.norm.* stay None without norm_embeddings
_TORCH_WRITTEN = ('model.cls_token', 'model.patch_embed.proj.bias', 'flag_post_linear.bias', 'model.norm.weight', 'model.norm.bias')


@pytest.mark.parametrize('precision,spec', [(p, s) for p in ('bf16', 'fp32') for s in ('1', '2,1', '3')] + [('fp16', '2,1')])
def test_backward_publishes_only_finished_buckets(precision, spec, monkeypatch):
    """CPU guard on engine.run_backward's ordering (the GPU tests check the values): the real backward on CPU tensors with a recording library
    and a recording hook (tests/engine_trace.py).  bf16 / fp16 fold the temporal projection (late bucket), fp32 does not; fp16 with an active
    hook makes publish() undo the loss scale."""
    import engine_trace as kit
    monkeypatch.setenv('TCOW_DDP_GROUP', spec)
    trace = kit.install(monkeypatch)
    net = kit.make_net(precision)
    m = kit.train_step(net, hook=kit.RecordingHook(trace), trace=trace)
    ev = list(trace.events)
    fold = precision != 'fp32'
    pubs = [(k, e[1], e[2]) for k, e in enumerate(ev) if e[0] == 'publish']
    touches = lambda e, lo, hi: e[0] == 'call' and any(lo <= p < hi for p in e[2])
    # the buckets come in the order g<top> ..., 'fold', 'g0'; the drain is the last event, right behind the bottom bucket
    assert [t for _, t, _ in pubs] == _bucket_tags(kit.DEPTH, spec, fold)
    assert ev[-1] == ('finish',) and ev[pubs[-1][0] + 1:] == [('finish',)]
    assert sum(e[0] == 'finish' for e in ev) == 1
    assert m.pending_inv_scale is None                                      # (fp16: the hook is active, so publish() unscaled every bucket itself)
    for k, tag, (lo, hi) in pubs:
        # a published bucket is finished: no library call receives a pointer into it any more
        late = [e[1] for e in ev[k + 1:] if touches(e, lo, hi)]
        assert not late, (tag, late)
        before = [e[1] for e in ev[:k] if touches(e, lo, hi)]
        if tag == 'fold':
            # the late bucket: right behind the four batched launches of _GradBuckets.finish_late, all of which write into it
            assert [e[1] for e in ev[k - 4:k]] == ['tcow_sgemm_x3_batched'] * 4 and all(touches(e, lo, hi) for e in ev[k - 4:k])
        else:
            # a block group (the bottom one included): its deferred weight-gradient GEMMs and LayerNorm folds were flushed before
            assert 'tcow_gemm_tn_grouped' in before and 'tcow_layernorm_fold' in before, (tag, before)
    # every parameter's gradient lies in exactly one published bucket, and a library call wrote into it before that bucket went out
    names = {id(p): n for n, p in net.named_parameters()}
    for p in m.param_list():
        name, gr = names[id(p)], p.grad
        if gr is None:
            assert name.endswith(('model.norm.weight', 'model.norm.bias')), name
            continue
        a = gr.data_ptr()
        home = [k for k, _, (lo, hi) in pubs if lo <= a and a + gr.numel() * 4 <= hi]
        assert len(home) == 1, (name, home)
        written = any(touches(e, a, a + gr.numel() * 4) for e in ev[:home[0]])
        assert written or name.endswith(_TORCH_WRITTEN), name


def test_hook_sees_complete_buckets_with_a_fake_engine_run(monkeypatch):
    """The same ordering with the real hook: engine.run_backward on CPU tensors (tests/engine_trace.py) drives a GradSync of one rank, and
    finish() leaves nothing pending before gradients are handed out (single process: the hook is a no-op but its state machine still runs)."""
    import engine_trace as kit
    from tcow_amd import ddp
    trace = kit.install(monkeypatch)
    sync = ddp.GradSync(1, force=False)
    m = kit.train_step(kit.make_net('bf16'), hook=sync)
    assert any(c[0] == 'tcow_gemm_tn_grouped' for c in trace.calls) and all(p.grad is not None for p in m.param_list()[:5])
    assert sync.pending == [] and sync.deferred == [] and sync.steps == 1
