"""Per-iteration summaries (audiogan_amd.summary.Summary; train.d_step_full / g_step_full(summary=...); loop.TrainLoop(summary=...)):
the reference's scalars of audiogan.py:776-809, :875-884, :911-920 computed by library kernels, gathered into a device ring
and read by the host in one copy - which is also the health check of a captured loop.  CPU: host logic on the kernel model
plus tests/summary_model.py; -m gpu: the HIP kernels."""
import collections
import json
import os

import numpy as np
import pytest
import torch

from oracle import audiogan_oracle as O
from tests import kernel_model, summary_model
from tests import step_fixture as SF
from tests.test_loop import _setup


def _install(monkeypatch):
    kernel_model.install(monkeypatch)
    summary_model.install(monkeypatch)


# ---- (1) / (6): the reference's own values ---------------------------------------------------------------------------
def _oracle_reward(v, monkeypatch):
    """per-sample losses of the generator iteration (audiogan.py:864) from the oracle driven through the fixture"""
    seen = []
    orig = O._masked_bce

    def rec(*a, **k):
        r = orig(*a, **k)
        seen.append(r.detach().double().numpy().copy())
        return r
    monkeypatch.setattr(O, '_masked_bce', rec)
    cpu = torch.device('cpu')
    g, d, e_g, e_d = mods = SF.build(O, v, cpu)
    opt_g = O.make_optimizer(list(g.parameters()) + list(e_g.parameters()), 'rmsprop', 1e-4)
    opt_d = O.make_optimizer(list(d.parameters()) + list(e_d.parameters()), 'rmsprop', 1e-4)
    mark = []

    def g_full(*a, **k):
        mark.append(len(seen))
        return O.g_step_full(*a, **k)
    SF.run(v, mods, opt_d, opt_g, O.d_step_full, g_full, cpu, rtol=1e-4, atol_scale=1e-5, post_atol=1e-4)
    monkeypatch.setattr(O, '_masked_bce', orig)
    ps = seen[-1]                              # (the last call inside g_step_full: ``loss_ps``)
    assert len(seen) > mark[0] and ps.shape == (v['g1.real'].shape[0],)
    np.testing.assert_allclose(ps.mean(), float(v['g1.bce']), rtol=1e-4)
    return -ps


def _fixture_rows(dev, A, golden_dir, monkeypatch, rtol, atol_scale):
    """``step_fixture.run`` with ``summary`` on (it also compares every stored result at the tolerances of
    test_full_step_reference_fixture_*: the summaries changed none of them), then the three rows against what the REFERENCE's
    loop body wrote into tests/golden/ref_step.npz, at ``rtol`` / ``atol_scale``"""
    from audiogan_amd import optim, train
    from audiogan_amd.summary import Summary
    v = SF.load(golden_dir)
    g, d, e_g, e_d = mods = SF.build(A, v, dev)
    opt_g = optim.make_optimizer(list(g.parameters()) + list(e_g.parameters()), 'rmsprop', 1e-4)
    opt_d = optim.make_optimizer(list(d.parameters()) + list(e_d.parameters()), 'rmsprop', 1e-4)
    S = Summary(dev, capacity=8)
    res = []

    def d_full(*a, **k):
        res.append(train.d_step_full(*a, summary=S, **k))
        return res[-1]

    def g_full(*a, **k):
        res.append(train.g_step_full(*a, summary=S, gen_iter=1, **k))
        return res[-1]
    agree = SF.run(v, mods, opt_d, opt_g, d_full, g_full, dev, rtol=1e-3, atol_scale=1e-4, post_atol=2e-3)
    assert agree > 0.99
    rows = S.drain()
    assert [(r['kind'], r['iter']) for r in rows] == [('D', 1), ('D', 2), ('G', 1)]
    for it, r in ((1, rows[0]), (2, rows[1])):
        pre = 'd%d.' % it
        print(pre, {k: r[k] for k in ('x_grad_norm', 'cls_d/mean', 'cls_d/std', 'cls_g/mean', 'cls_g/std', 'd_grad_norm')},
              float(v[pre + 'x_grad_norm']))
        # a squared norm: twice the gradients' tolerance
        np.testing.assert_allclose(r['x_grad_norm'], float(v[pre + 'x_grad_norm']), rtol=2 * rtol)
        for k in ('loss', 'loss_d', 'loss_g'):
            SF._close(r[k], v[pre + k], rtol, atol_scale, pre + k)
        for tag in ('cls_d', 'cls_g'):
            ref = v[pre + tag].astype(np.float64)
            SF._close(r[tag + '/mean'], ref.mean(), rtol, atol_scale, pre + tag + '/mean')
            # |std(x) - std(y)| <= max |x - y|: the logits' own allowance
            amax = float(np.abs(ref).max())
            assert abs(r[tag + '/std'] - ref.std()) <= atol_scale * max(1e-3, amax) + rtol * amax, (tag, r[tag + '/std'], ref.std())
        np.testing.assert_allclose([r['acc_d'], r['acc_g']], v[pre + 'acc'], atol=1e-6)
        np.testing.assert_allclose(r['d_grad_norm'], float(v[pre + 'grad_norm']), rtol=max(rtol, 1e-4))
    r, pre = rows[2], 'g1.'
    loose = max(rtol, 2e-3) if agree < 1.0 else rtol
    la = max(atol_scale, 1e-4 if agree < 1.0 else 0)
    print(pre, r)
    SF._close(r['reward/mean'], -float(v[pre + 'bce']), loose, la, 'reward/mean')
    for k in ('bce', 'feature_penalty', 'loss'):
        SF._close(r[k], v[pre + k], loose, la, pre + k)
    assert abs(r['reward_baseline'] - float(v[pre + 'baseline'])) <= loose * abs(float(v[pre + 'baseline'])) + 1e-7
    np.testing.assert_allclose(r['g_grad_norm'], float(v[pre + 'grad_norm']), rtol=max(loose, 1e-4))
    assert r['lambda_fp'] == 1.0
    # reward/std against the oracle's per-sample losses: each of them is within ``loose`` of the product's (the allowance of
    # ``bce``, their mean), and a std moves by at most the largest change of an element
    rw = _oracle_reward(v, monkeypatch)
    amax = float(np.abs(rw).max())
    assert abs(r['reward/std'] - rw.std()) <= loose * amax + la * max(1e-3, amax), (r['reward/std'], rw.std())
    # the tensors behind the rows, recomputed on the host
    B = res[0]['x_grad'].size(0)
    for it in (0, 1):
        xg, nf = res[it]['x_grad'].detach().double().cpu(), res[it]['nf_g'].double().cpu()
        np.testing.assert_allclose(rows[it]['x_grad_norm'], float((B * B * (xg ** 2).sum(1) / nf).mean()), rtol=1e-5)
    return rows


def test_reference_fixture_summaries_host_logic(monkeypatch, golden_dir):
    _install(monkeypatch)
    import audiogan_amd as A
    _fixture_rows(torch.device('cpu'), A, golden_dir, monkeypatch, 1e-4, 1e-5)


@pytest.mark.gpu
def test_reference_fixture_summaries_gpu(monkeypatch, golden_dir):
    """the tolerances of test_full_step_reference_fixture_gpu (1e-3; 2e-3 for the squared norm)"""
    import audiogan_amd as A
    _fixture_rows(torch.device('cuda'), A, golden_dir, monkeypatch, 1e-3, 1e-4)


# ---- (2): the ring -----------------------------------------------------------------------------------------------------
def _commit(S, kind, it, val):
    S.commit(kind, it, {2: torch.tensor([val], device=S.dev), 4: float(val) + 0.5, 13: torch.zeros(1, dtype=torch.int32, device=S.dev)})


def test_ring_order_wrap_and_auto_drain(monkeypatch, tmp_path):
    _install(monkeypatch)
    from audiogan_amd.summary import Summary
    got = []
    path = os.path.join(tmp_path, 'rows.jsonl')
    S = Summary(torch.device('cpu'), capacity=4, on_row=got.append, path=path)
    assert S.drain() == []
    for i in range(3):
        _commit(S, 0, i + 1, float(i))
    rows = S.drain()
    assert [(r['kind'], r['iter'], r['loss_d'], r['loss']) for r in rows] == [('D', 1, 0.0, 0.5), ('D', 2, 1.0, 1.5), ('D', 3, 2.0, 2.5)]
    # rows 3, 0, 1 of the ring: the wrap keeps the order
    _commit(S, 1, 1, 10.0); _commit(S, 0, 4, 11.0); _commit(S, 1, 2, 12.0)
    rows = S.drain()
    assert [(r['kind'], r['iter'], r['bce'] if r['kind'] == 'G' else r['loss_d']) for r in rows] == \
        [('G', 1, 10.0), ('D', 4, 11.0), ('G', 2, 12.0)]
    assert int(S.cursor[0]) == 2 and int(S.cursor[1]) == 6 and len(got) == 6
    # a full ring is drained before the next row would overwrite an unseen one
    for i in range(4):
        _commit(S, 0, 5 + i, 20.0 + i)
    assert len(got) == 6 and len(S.pending) == 4
    _commit(S, 0, 9, 24.0)
    assert len(got) == 10 and len(S.pending) == 1 and [r['iter'] for r in got[6:]] == [5, 6, 7, 8]
    assert [r['iter'] for r in S.drain()] == [9]
    lines = [json.loads(s) for s in open(path).read().splitlines()]
    assert lines == got and len(lines) == 11
    # a row the host did not expect is a gap, not a silent loss
    _commit(S, 0, 10, 1.0)
    S.cursor[1] += 1
    with pytest.raises(RuntimeError, match='rows were lost'):
        S.drain()


def test_loop_commits_every_iteration_and_run_drains(monkeypatch, tmp_path):
    _install(monkeypatch)
    import audiogan_amd as A
    from audiogan_amd.summary import Summary
    got = []
    path = os.path.join(tmp_path, 'rows.jsonl')
    S = Summary(torch.device('cpu'), capacity=4, on_row=got.append, path=path)
    mk, mods, _ = _setup(A, torch.device('cpu'), False, tmp_path, 4)
    lp = mk(fixed_critic_iter=2, gencatchup=1, stop='never', checkpoint_every=0, check=False, host=False, summary=S,
            summary_every=100)
    lp.run(3)
    assert S.pending == [] and lp.dis_iter == 6 and lp.gen_iter == 3
    assert [(r['kind'], r['iter']) for r in got] == [('D', 1), ('D', 2), ('G', 1), ('D', 3), ('D', 4), ('G', 2), ('D', 5), ('D', 6),
                                                   ('G', 3)]
    assert len(open(path).read().splitlines()) == 9
    for r in got:
        assert all(np.isfinite(x) for k, x in r.items() if k not in ('kind', 'iter')), r
        if r['kind'] == 'D':
            assert 0.0 <= r['acc_d'] <= 1.0 and r['x_grad_norm'] > 0.0 and r['cls_d/std'] > 0.0
            np.testing.assert_allclose(r['loss'], r['loss_d'] + r['loss_g'], rtol=1e-6)
        else:
            np.testing.assert_allclose(r['reward/mean'], -r['bce'], rtol=1e-5)
            np.testing.assert_allclose(r['loss'], r['bce'] + r['feature_penalty'] * r['lambda_fp'], rtol=1e-5)
    # summary_every: the loop drains on its own
    got[:] = []
    lp.summary_every = 2
    lp.outer()
    assert [(r['kind'], r['iter']) for r in got] == [('D', 7), ('D', 8)] and len(S.pending) == 1


# ---- (3): health -------------------------------------------------------------------------------------------------------
def test_nan_parameter_raises_at_the_drain_and_no_checkpoint_is_written(monkeypatch, tmp_path):
    _install(monkeypatch)
    import audiogan_amd as A
    from audiogan_amd.summary import Summary
    S = Summary(torch.device('cpu'), capacity=16)
    mk, mods, prefix = _setup(A, torch.device('cpu'), False, tmp_path, 4)
    lp = mk(fixed_critic_iter=2, gencatchup=1, stop='never', checkpoint_every=1, check=False, host=False, summary=S)
    lp.outer()
    assert os.path.exists('%s-dis-%05d' % (prefix, 1)) and S.pending == []
    with torch.no_grad():
        next(mods[1].parameters()).view(-1)[0] = float('nan')
    with pytest.raises(AssertionError, match=r'NaN in gradients \(check_grad\)'):
        lp.outer()
    assert lp.gen_iter == 2
    for role in ('dis', 'gen', 'eg', 'ed', 'opt'):
        assert not os.path.exists('%s-%s-%05d' % (prefix, role, 2))


# ---- (4): summary off ----------------------------------------------------------------------------------------------------
def _record_calls(monkeypatch):
    import audiogan_amd.kernels as K
    calls = []

    def wrap(name, fn):
        def rec(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return rec
    for n in set(kernel_model.ALL) | set(summary_model.ALL):
        f = getattr(K, n)
        if callable(f) and not isinstance(f, type) and not n.endswith('_ok'):      # (launches, not the dispatch predicates)
            monkeypatch.setattr(K, n, wrap(n, f))
    return calls


def _subsequence(a, b):
    it = iter(b)
    return all(x in it for x in a)


def test_summary_off_issues_the_same_kernel_calls(monkeypatch, golden_dir):
    """without ``summary`` d_step_full / g_step_full call ``kernels.*`` exactly as they do when nobody asks for summaries: the
    calls with ``summary`` on are the same sequence plus the summary kernels and ONE backward-data pass per critic iteration"""
    _install(monkeypatch)
    import audiogan_amd as A
    from audiogan_amd import optim, train
    from audiogan_amd.summary import Summary
    calls = _record_calls(monkeypatch)
    v = SF.load(golden_dir)
    cpu = torch.device('cpu')
    seqs = []
    for S in (None, Summary(cpu, capacity=8)):
        g, d, e_g, e_d = mods = SF.build(A, v, cpu)
        opt_g = optim.make_optimizer(list(g.parameters()) + list(e_g.parameters()), 'rmsprop', 1e-4)
        opt_d = optim.make_optimizer(list(d.parameters()) + list(e_d.parameters()), 'rmsprop', 1e-4)
        kw = dict(summary=S) if S is not None else {}
        calls[:] = []
        SF.run(v, mods, opt_d, opt_g, lambda *a, **k: train.d_step_full(*a, **kw, **k),
               lambda *a, **k: train.g_step_full(*a, **kw, **k), cpu)
        seqs.append(list(calls))
    off, on = seqs
    assert not set(off) & set(summary_model.ALL) and len(off) > 100
    extra = collections.Counter(on) - collections.Counter(off)
    assert extra == collections.Counter(logit_summary=4, sqnorm_rows=2, vec_stats=1, summary_commit=3, conv_engine=2), extra
    assert not collections.Counter(off) - collections.Counter(on)
    assert _subsequence(off, on)


# ---- (5): each kernel against float64 numpy ------------------------------------------------------------------------------
def _ref_logits(x, nf, positive):
    x = x.astype(np.float64)
    B, T = x.shape
    mask = np.arange(T)[None, :] < nf[:, None]
    hit = ((x > 0) if positive else (x < 0)) & mask
    return np.array([x.mean(), x.std(), hit.sum(), mask.sum(), hit.sum() / mask.sum()])


@pytest.mark.gpu
@pytest.mark.parametrize('B,T', [(64, 128), (3, 5)])
def test_logit_summary_kernel_gpu(B, T):
    import audiogan_amd.kernels as K
    gen = torch.Generator().manual_seed(100 + B)
    # the heads' layout: [T', B] rows handed on as a transposed view (``Discriminator.classify``); a narrow spread on an offset,
    # like real logits
    base = (torch.randn(T, B, generator=gen) * 0.05 + 0.03).cuda()
    cls = base.view(T, B).t()
    assert cls.stride() == (1, B)
    nf = torch.randint(1, T + 1, (B,), generator=gen)
    nf[0], nf[1] = 1, T                             # a clip of length 1
    nfd = nf.cuda()
    for positive in (True, False):
        out = K.logit_summary(cls, nfd, positive)
        ref = _ref_logits(cls.cpu().numpy(), nf.numpy(), positive)
        print(B, T, positive, out.cpu().numpy(), ref)
        np.testing.assert_allclose(out.cpu().numpy().astype(np.float64), ref, rtol=1e-5)
        assert torch.equal(out, K.logit_summary(cls, nfd, positive))
        # a contiguous copy gives the same numbers (the other index order)
        np.testing.assert_allclose(K.logit_summary(cls.contiguous(), nfd, positive).cpu().numpy().astype(np.float64), ref, rtol=1e-5)
    with pytest.raises(TypeError):
        K.logit_summary(cls.double(), nfd, True)
    with pytest.raises(RuntimeError):
        K.logit_summary(cls.cpu(), nfd, True)


@pytest.mark.gpu
def test_sqnorm_rows_kernel_gpu():
    import audiogan_amd.kernels as K
    gen = torch.Generator().manual_seed(7)
    B, L = 64, 8192
    for pitch, off in ((L + 24, 0), (L + 3, 1)):           # 16-byte aligned rows, and rows that are not
        buf = (torch.randn(B * pitch + 8, generator=gen) * 1e-3).cuda()
        gx = buf[off:off + B * pitch].view(B, pitch)[:, :L]
        nf = torch.randint(1, 129, (B,), generator=gen)
        nf[0] = 1
        nfd = nf.cuda()
        part, out = K.sqnorm_rows(gx, nfd, 4096.0)
        x = gx.cpu().numpy().astype(np.float64)
        ref = 4096.0 * (x ** 2).sum(1) / nf.numpy()
        print(pitch, float(out), ref.mean())
        np.testing.assert_allclose(part.cpu().numpy().astype(np.float64), ref, rtol=1e-5)
        np.testing.assert_allclose(float(out), ref.mean(), rtol=1e-5)
        part2, out2 = K.sqnorm_rows(gx, nfd, 4096.0)
        assert torch.equal(part, part2) and torch.equal(out, out2)
    with pytest.raises(AssertionError):
        K.sqnorm_rows(gx.t(), nfd, 1.0)


@pytest.mark.gpu
def test_vec_stats_and_commit_kernels_gpu():
    import audiogan_amd.kernels as K
    gen = torch.Generator().manual_seed(9)
    for n in (64, 5, 1):
        v = (torch.randn(n, generator=gen) * 0.01 + 0.7).cuda()
        out = K.vec_stats(v, -1.0)
        x = v.cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(out.cpu().numpy().astype(np.float64), [-x.mean(), x.std()], rtol=1e-5, atol=1e-12)
        assert torch.equal(out, K.vec_stats(v, -1.0))
    # the commit: floats and integers keep their bits, column 1 is the sequence number, the cursor wraps
    K.reserve_table_arena()
    rings = []
    for _ in range(2):
        ring = torch.zeros(3, 16, dtype=torch.int32, device='cuda')
        cur = torch.zeros(2, dtype=torch.int32, device='cuda')
        f = torch.tensor([1.25, -3.5e-7], device='cuda')
        flags = torch.tensor([3], dtype=torch.int32, device='cuda')
        part = torch.tensor([0.1, 0.2, 0.4], device='cuda')
        for i in range(4):
            K.summary_commit(ring, cur, [i % 2, 99, f[0:1], f[1:2], 2.5, None, None, None, None, None, None, None, None, flags,
                                         -2, None], part=part, part_col=12)
        rings.append((ring.cpu(), cur.cpu()))
    ring, cur = rings[0]
    assert cur.tolist() == [1, 4]
    assert ring[:, 0].tolist() == [1, 1, 0] and ring[:, 1].tolist() == [3, 1, 2]
    fl = ring.view(torch.float32)
    assert float(fl[1, 2]) == 1.25 and float(fl[1, 3]) == float(np.float32(-3.5e-7)) and float(fl[1, 4]) == 2.5
    assert int(ring[1, 13]) == 3 and int(ring[1, 14]) == -2
    assert ring[1, 5:12].abs().sum() == 0 and ring[1, 15] == 0
    np.testing.assert_allclose(float(fl[1, 12]), (np.float64(np.float32(0.1)) + np.float32(0.2) + np.float32(0.4)) / 3, rtol=1e-6)
    assert torch.equal(rings[0][0], rings[1][0]) and torch.equal(rings[0][1], rings[1][1])
    # the same mean as the norm kernel's finishing launch, bit for bit
    gx = torch.randn(5, 64, generator=gen).cuda()
    nf = torch.tensor([3, 1, 4, 1, 5]).cuda()
    p, out = K.sqnorm_rows(gx, nf, 25.0)
    ring.zero_()
    ring, cur = ring.cuda(), torch.zeros(2, dtype=torch.int32, device='cuda')
    K.summary_commit(ring, cur, [None] * 16, part=p, part_col=12)
    assert torch.equal(ring[0, 12:13].view(torch.float32), out)


# ---- (7): C2 widths, every row value against float64 torch -----------------------------------------------------------------
@pytest.mark.gpu
def test_rows_at_c2_widths_gpu(tmp_path):
    import audiogan_amd as A
    from audiogan_amd import kernels as K
    from audiogan_amd.summary import Summary
    dev = torch.device('cuda')
    K.lstm_persist_status(reset=True)
    S = Summary(dev, capacity=8)
    mk, mods, _ = _setup(A, dev, True, tmp_path, 8)
    torch.cuda.manual_seed(3)
    # Bernoulli stop draws: ragged generated clips beside the loader's ragged real clips
    lp = mk(fixed_critic_iter=2, gencatchup=1, stop=None, checkpoint_every=0, check=True, host=False, summary=S)
    res = []
    for step in (lp.d_iteration, lp.d_iteration, lp.g_iteration):
        r = step()
        # (``grad_norm`` is the optimiser's own norm_sum tensor, which the next step of that optimiser overwrites: read it now)
        res.append(dict(r, grad_norm=float(r['grad_norm'])))
    rows = S.drain()
    assert [(r['kind'], r['iter']) for r in rows] == [('D', 1), ('D', 2), ('G', 1)]
    f64 = lambda t: t.detach().double().cpu()  # noqa: E731
    B = 8
    for r, row in zip(res[:2], rows[:2]):
        want = {'loss': float(r['loss']), 'loss_d': float(r['loss_d']), 'loss_g': float(r['loss_g']),
                'd_grad_norm': float(r['grad_norm'])}
        for tag, nf, pos in (('d', r['nf_d'], True), ('g', r['nf_g'], False)):
            x = f64(r['cls_' + tag])
            want['cls_%s/mean' % tag] = float(x.mean())
            want['cls_%s/std' % tag] = float(x.std(unbiased=False))
            w = (torch.arange(x.size(1)).view(1, -1) < nf.cpu().view(-1, 1)).double()
            want['acc_' + tag] = float(((((x > 0) if pos else (x < 0)).double()) * w).sum() / w.sum())
            assert row['acc_' + tag] == float(r['acc_' + tag])
        xg = f64(r['x_grad'])
        assert xg.shape[0] == B and float(xg.abs().max()) > 0
        want['x_grad_norm'] = float((B * B * (xg ** 2).sum(1) / r['nf_g'].double().cpu()).mean())
        print(row, want)
        for k, w_ in want.items():
            np.testing.assert_allclose(row[k], w_, rtol=1e-4, err_msg=k)
    r, row = res[2], rows[2]
    rw = f64(r['reward'])
    want = {'bce': float(r['bce']), 'feature_penalty': float(r['feature_penalty']), 'loss': float(r['loss']),
            'reward/mean': float(rw.mean()), 'reward/std': float(rw.std(unbiased=False)), 'reward_baseline': float(r['baseline']),
            'g_grad_norm': float(r['grad_norm']), 'lambda_fp': 1.0}
    print(row, want)
    for k, w_ in want.items():
        np.testing.assert_allclose(row[k], w_, rtol=1e-4, err_msg=k)
    np.testing.assert_allclose(row['reward/mean'], -row['bce'], rtol=1e-4)
    assert K.lstm_persist_status() == 0


# ---- (8): summaries change no training bit -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_summaries_change_no_training_bit_gpu(tmp_path):
    """12 critic + 6 generator iterations at the C2 widths, eager and captured, with and without a summary: the same bits in
    every parameter; the captured loop's rows are the eager loop's rows exactly"""
    import audiogan_amd as A
    from audiogan_amd import kernels as K
    from audiogan_amd.summary import Summary
    dev = torch.device('cuda')
    K.lstm_persist_status(reset=True)
    got = {}
    for graphed in (False, True):
        for on in (False, True):
            rows = []
            S = Summary(dev, capacity=8, on_row=rows.append) if on else None
            mk, mods, _ = _setup(A, dev, True, tmp_path, 8)
            torch.cuda.manual_seed(17)
            lp = mk(fixed_critic_iter=2, gencatchup=1, stop='never', checkpoint_every=0, check=False, graphed=graphed, host=False,
                    **(dict(summary=S) if on else {}))
            # (the first captured call runs two eager passes as its warm-up - real training iterations, counted)
            n = 4 if graphed else 6
            for _ in range(n - 1):
                lp.outer()
            lp.run(1)
            assert lp.dis_iter == 12 and lp.gen_iter == 6
            if graphed:
                assert lp._graphs is not None
            if on:
                assert S.pending == [] and len(rows) == 18
            got[graphed, on] = ([p.detach().clone() for m in mods for p in m.parameters()], rows)
    assert K.lstm_persist_status() == 0
    for key in ((False, True), (True, False), (True, True)):
        for p, q in zip(got[False, False][0], got[key][0]):
            assert torch.equal(p, q), key
    eager, cap = got[False, True][1], got[True, True][1]
    assert [(r['kind'], r['iter']) for r in eager] == [('D', 1), ('D', 2), ('G', 1), ('D', 3), ('D', 4), ('G', 2), ('D', 5), ('D', 6),
                                                     ('G', 3), ('D', 7), ('D', 8), ('G', 4), ('D', 9), ('D', 10), ('G', 5), ('D', 11),
                                                     ('D', 12), ('G', 6)]
    assert eager == cap
    for r in eager:
        assert all(np.isfinite(x) for k, x in r.items() if k not in ('kind', 'iter')), r


# ---- (9): health of a captured loop -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_captured_loop_health_gpu(tmp_path):
    """a captured loop looks at its own health at every drain: a sticky status word (set here by a host-side write into the
    workspace - no launch misbehaves) raises PersistentLaunchError and is reset, a NaN critic parameter raises the check_grad
    assertion; in both cases the checkpoint of that iteration is not written"""
    import audiogan_amd as A
    from audiogan_amd import kernels as K
    from audiogan_amd.summary import Summary
    dev = torch.device('cuda')
    K.lstm_persist_status(reset=True)
    S = Summary(dev, capacity=32)
    mk, mods, prefix = _setup(A, dev, True, tmp_path, 8)
    torch.cuda.manual_seed(5)
    lp = mk(fixed_critic_iter=2, gencatchup=1, stop='never', checkpoint_every=0, check=False, graphed=True, host=False, summary=S)
    lp.outer()                                   # two warm-up passes, the captures, one replayed pass
    assert lp._graphs is not None and lp.gen_iter == 3
    lp.checkpoint_every = 1
    lp.outer()
    assert os.path.exists('%s-dis-%05d' % (prefix, 4)) and S.pending == []
    word = K.persist_status_word(dev)
    assert word is not None and int(word.item()) == 0
    word.copy_(torch.tensor([5], dtype=torch.int32))
    with pytest.raises(K.PersistentLaunchError, match='status 0x00000005'):
        lp.outer()
    assert K.lstm_persist_status() == 0 and lp.gen_iter == 5 and S.pending == []
    assert not os.path.exists('%s-dis-%05d' % (prefix, 5))
    lp.outer()                                   # the run is healthy again
    assert os.path.exists('%s-dis-%05d' % (prefix, 6))
    with torch.no_grad():
        next(mods[1].parameters()).view(-1)[0] = float('nan')
    with pytest.raises(AssertionError, match=r'NaN in gradients \(check_grad\)'):
        lp.outer()
    assert lp.gen_iter == 7 and not os.path.exists('%s-dis-%05d' % (prefix, 7))
    assert K.lstm_persist_status() == 0


# ---- (10): launch budget ---------------------------------------------------------------------------------------------------------
class _AtenOps(torch.utils._python_dispatch.TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops = collections.Counter()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.ops[str(func)] += 1
        return func(*args, **(kwargs or {}))


@pytest.mark.gpu
def test_launch_budget_gpu(golden_dir):
    """counted with K.Profiler: a critic iteration with ``summary`` adds at most 4 library launches beyond the first layer's
    backward-data pass, a generator iteration at most 3; and no statistic comes from a torch op (no reduction, comparison or
    arithmetic aten op is added on the calling thread)"""
    import audiogan_amd as A
    from audiogan_amd import kernels as K, optim, train
    from audiogan_amd.summary import Summary
    dev = torch.device('cuda')
    v = SF.load(golden_dir)
    counts = {}
    for on in (False, True):
        g, d, e_g, e_d = mods = SF.build(A, v, dev)
        opt_g = optim.make_optimizer(list(g.parameters()) + list(e_g.parameters()), 'rmsprop', 1e-4)
        opt_d = optim.make_optimizer(list(d.parameters()) + list(e_d.parameters()), 'rmsprop', 1e-4)
        kw = dict(summary=Summary(dev, capacity=8)) if on else {}
        profs = []

        def prof(fn):
            def run(*a, **k):
                K.Profiler.start()
                try:
                    with _AtenOps() as ops:
                        return fn(*a, **kw, **k)
                finally:
                    p = K.Profiler.stop()
                    profs.append((collections.Counter({n: r['n'] for n, r in p.items()}), ops.ops))
            return run
        SF.run(v, mods, opt_d, opt_g, prof(train.d_step_full), prof(train.g_step_full), dev, rtol=1e-3, atol_scale=1e-4,
               post_atol=2e-3)
        counts[on] = profs
    names = {'logit_summary_kernel', 'sqnorm_rows_kernel', 'vec_stats_kernel', 'summary_commit_kernel'}
    stat_ops = ('mean', 'std', 'var', 'sum', 'pow', 'sqrt', 'norm', 'div', 'mul', 'sub', 'add', 'gt', 'lt', 'where', 'item',
                '_local_scalar_dense')
    for i, budget in ((0, 4), (1, 4), (2, 3)):
        (k_off, a_off), (k_on, a_on) = counts[False][i], counts[True][i]
        extra = k_on - k_off
        print(i, dict(extra), dict(a_on - a_off))
        assert not k_off - k_on and not set(k_off) & names
        own = collections.Counter({n: c for n, c in extra.items() if n in names})
        other = extra - own
        assert sum(own.values()) <= budget, extra
        if i < 2:
            assert own == collections.Counter(logit_summary_kernel=2, sqnorm_rows_kernel=1, summary_commit_kernel=1), extra
            assert sum(other.values()) == 1 and all(n.startswith('conv') for n in other), extra      # the backward-data pass
        else:
            assert own == collections.Counter(vec_stats_kernel=1, summary_commit_kernel=1) and not other, extra
        for op in a_on - a_off:
            assert not any(op.startswith('aten.%s.' % s) or op.startswith('aten.%s_.' % s) for s in stat_ops), (i, op)
