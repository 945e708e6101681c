"""evaluate.Evaluator: held-out critic scores and the spectral distance of the samples (kernels.ltas_power / ag_ltas_power,
kernels.score_accum / ag_score_accum), TrainLoop(evaluator=..., eval_every=...) and Discriminator.refresh_weights.
CPU: host logic on the kernel models (tests/kernel_model.py + tests/eval_model.py); -m gpu: the HIP kernels, eager and between
the replays of a captured loop.

Bounds.  ltas_power: |P - P64| <= 2e-5 max_k P64[b] per clip against float64 numpy (np.fft.rfft).  score_accum: counts exact,
the loss word 1e-6 relative (fp32 softplus terms, all positive, summed in double), the two moment words 1e-12 relative.
Evaluator.run against a float64 restatement from the tensors it returns: losses 1e-6 relative (the same fp32 terms), the
other critic numbers 1e-9 (float64 sums of the same fp32 logits, in another order), feature_penalty 1e-5 relative against the
unfused form, ltas_db 1e-4 dB."""
import collections
import json
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import eval_model, kernel_model
from tests.eval_model import (LTAS_FRAMES, LTAS_KINDS, LTAS_L, check_ltas, check_scores, ltas_case, score_accum64,
                              score_case)

CFGS = dict(
    # the configs of tests/test_ema.py (CPU) ...
    toy=dict(frame=32, maxlen=128,
             g=dict(frame_size=32, embed_size=8, noise_size=8, state_size=64, num_layers=1, struct=[[17, 8, 16, 8], [9, 4, 16, 8]]),
             d=dict(state_size=64, embed_size=8, num_layers=1, cnn_struct=[[7, 2, 8], [7, 2, 16]]),
             e=dict(output_size=8, char_embed_size=6, num_chars=256)),
    # ... its GPU loop's (S = 128, fs = 40: the fronts' persistent launches take them) ...
    toy_gpu=dict(frame=40, maxlen=320,
                 g=dict(frame_size=40, embed_size=8, noise_size=8, state_size=128, num_layers=1, struct=[[17, 8, 16, 8], [9, 4, 16, 8]]),
                 d=dict(state_size=64, embed_size=8, num_layers=1, cnn_struct=[[7, 2, 8], [7, 2, 16]]),
                 e=dict(output_size=8, char_embed_size=6, num_chars=256)),
    # ... and the C2 widths of tests/test_loop.py
    c2=dict(frame=256, maxlen=8192,
            g=dict(frame_size=256, embed_size=100, noise_size=100, state_size=1024, num_layers=1),
            d=dict(state_size=1024, embed_size=100, num_layers=1),
            e=dict(output_size=100, char_embed_size=50, num_layers=1, num_chars=256)))
FLOATS = ('loss_d', 'acc_d', 'cls_d/mean', 'cls_d/std', 'loss_g', 'acc_g', 'cls_g/mean', 'cls_g/std', 'feature_penalty',
          'ltas_db', 'frames/mean')
INTS = ('clips', 'gen_iter', 'dis_iter')


def _models(monkeypatch):
    kernel_model.install(monkeypatch)
    eval_model.install(monkeypatch)


def _fresh(A, cfg, dev):
    c = CFGS[cfg]
    return (A.Generator(**c['g']).to(dev), A.Discriminator(**c['d']).to(dev), A.Embedder(**c['e']).to(dev),
            A.Embedder(**c['e']).to(dev))


def _setup(A, dev, cfg, tmp_path, B, batches=2):
    """tests.test_loop._setup, keeping the validation loader: ``batches`` held-out minibatches are taken from it BEFORE the
    training loader's first next() (dataset.py draws from the global numpy generator), whether an evaluator is built or not -
    so loops with and without one see the same training data"""
    from audiogan_amd import dataset as D
    from audiogan_amd import loop, optim
    torch.manual_seed(81)
    c = CFGS[cfg]
    g, d, e_g, e_d = mods = _fresh(A, cfg, dev)
    opt_g = optim.make_optimizer(list(g.parameters()) + list(e_g.parameters()), 'rmsprop', 1e-4)
    opt_d = optim.make_optimizer(list(d.parameters()) + list(e_d.parameters()), 'rmsprop', 1e-4)
    words = ['alpha', 'beta', 'gamma', 'delta', 'epsil', 'zetaa', 'etaaa', 'theta', 'iotaa', 'kappa', 'lambd']
    ds = D.SyntheticWordDataset(words, n_per_word=3, min_len=c['maxlen'] // 3, max_len=c['maxlen'], kind='noise', seed=3)
    args = types.SimpleNamespace(conditional=True, dataset=ds, minwordlen=1, subset=None, amplitudes=0)
    np.random.seed(5)
    h5, ml, gen_train, gen_valid, keys_train, _ = D.dataloader(B, args, maxlen=c['maxlen'], frame_size=c['frame'])
    heldout = [next(gen_valid) for _ in range(batches)]
    pick = loop.words_picker(D, B, ml, h5, keys_train, args, frame_size=c['frame'])
    mk = lambda **kw: loop.TrainLoop(g, d, e_g, e_d, opt_g, opt_d, gen_train, pick, B, ml, dev,  # noqa: E731
                                     checkpoint_prefix=os.path.join(tmp_path, 'run'), **kw)
    return types.SimpleNamespace(mk=mk, mods=mods, heldout=heldout, loader=gen_train, maxlen=ml, B=B, opt_g=opt_g, cfg=cfg,
                                 dev=dev)


def _evaluator(s, mods=None, **kw):
    from audiogan_amd.evaluate import Evaluator
    g, d, e_g, e_d = mods if mods is not None else s.mods
    return Evaluator(g, d, e_g, e_d, s.heldout, s.B, s.maxlen, s.dev, batches=len(s.heldout), seed=21, **kw)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _restate(res, parts, ev):
    """every metric of ``res`` from the returned parts, in float64"""
    from audiogan_amd import extras
    from audiogan_amd.evaluate import finish_scores
    fs, B = ev.g._frame_size, ev.B
    acc = dict(d=np.zeros(6), g=np.zeros(6))
    pen, dist, frames = [], [], []
    for p in parts:
        acc['d'] += score_accum64(p['cls_d'].cpu().numpy(), p['nf_d'].cpu().numpy(), 0.9, True)
        acc['g'] += score_accum64(p['cls_g'].cpu().numpy(), p['nf_g'].cpu().numpy(), 0.0, False)
        with torch.no_grad():
            pen.append(float(extras.feature_penalty(extras.calc_dists(p['hs_d'], p['hl_d']),
                                                    extras.calc_dists(p['hs_g'], p['hl_g']), B)))
        dbf = 10.0 * np.log10(p['power'].cpu().numpy().astype(np.float64) + 1e-10)
        dbr = 10.0 * np.log10(p['real_power'].cpu().numpy().astype(np.float64) + 1e-10)
        dist += list(np.sqrt(((dbf - dbr) ** 2).mean(1)))
        ln = p['length'].cpu().numpy()
        assert (ln % fs == 0).all() and p['wave'].size(1) == ln.max()
        frames += list(ln // fs)
    assert res['clips'] == len(dist) == B * len(parts)
    for tag in 'dg':
        loss, a, mean, std = finish_scores(acc[tag])
        got = [res['loss_' + tag], res['acc_' + tag], res['cls_%s/mean' % tag], res['cls_%s/std' % tag]]
        print('%s: got %s want %s' % (tag, got, [loss, a, mean, std]))
        assert _rel(got[0], loss) <= 1e-6 and _rel(got[1], a) <= 1e-12, (tag, got, loss, a)
        assert abs(got[2] - mean) <= 1e-9 * max(abs(mean), math.sqrt(acc[tag][5] / acc[tag][2])) and _rel(got[3], std) <= 1e-9
        assert 0.0 <= got[1] <= 1.0 and got[0] > 0 and got[3] > 0
    print('feature_penalty %r want %r; ltas_db %r want %r' % (res['feature_penalty'], np.mean(pen), res['ltas_db'], np.mean(dist)))
    assert _rel(res['feature_penalty'], float(np.mean(pen))) <= 1e-5
    assert abs(res['ltas_db'] - float(np.mean(dist))) <= 1e-4 and res['ltas_db'] > 0
    assert _rel(res['frames/mean'], float(np.mean(frames))) <= 1e-12 and res['frames/mean'] >= 1


def _run_checks(s, tmp_path):
    """Evaluator.run against the float64 restatement; the dict reaches on_eval and the JSON line unchanged; a second run
    gives the same bits; no generator, no .grad and no loader position moves"""
    seen = []
    path = os.path.join(tmp_path, 'eval.jsonl')
    ev = _evaluator(s, on_eval=seen.append, path=path)
    assert ev.clips == s.B * len(s.heldout) and len(ev.set) == len(s.heldout)
    state = (torch.random.get_rng_state(), np.random.get_state(),
             torch.cuda.get_rng_state() if s.dev.type == 'cuda' else None)
    res, parts = ev.run(gen_iter=7, dis_iter=19, parts=True)
    assert set(res) == set(FLOATS) | set(INTS) and (res['gen_iter'], res['dis_iter']) == (7, 19)
    assert all(isinstance(res[k], float) and math.isfinite(res[k]) for k in FLOATS) and isinstance(res['clips'], int)
    _restate(res, parts, ev)
    res2 = ev.run(gen_iter=7, dis_iter=19)
    assert res2 == res, (res, res2)
    assert seen == [res, res2] and seen[0] is not seen[1]
    with open(path) as f:
        lines = [json.loads(ln) for ln in f]
    assert lines == [dict(kind='E', **res), dict(kind='E', **res2)]
    assert torch.equal(torch.random.get_rng_state(), state[0])
    st = np.random.get_state()
    assert st[0] == state[1][0] and np.array_equal(st[1], state[1][1]) and st[2:] == state[1][2:]
    if state[2] is not None:
        assert torch.equal(torch.cuda.get_rng_state(), state[2])
    assert all(p.grad is None for m in s.mods for p in m.parameters())
    return ev, res


# ------------------------------------------------------------------------------------------------------------------
# CPU: kernel model + eval model
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', LTAS_KINDS)
def test_ltas_model_against_float64(kind):
    buf, lens = ltas_case(kind)
    nf = torch.zeros(len(lens), dtype=torch.int32)
    P = eval_model.ltas_power(buf[:, :LTAS_L], lens, nframes=nf)
    check_ltas(P, nf, buf, lens, LTAS_L, frames=LTAS_FRAMES)
    if kind == 'randn':
        buf, lens = ltas_case(kind, L=40000, ld=40000, lens=(40000,))
        check_ltas(eval_model.ltas_power(buf, lens), None, buf, lens, 40000, frames=(311,))
        buf, lens = ltas_case(kind, L=4096, ld=4099, lens=RAGGED)
        check_ltas(eval_model.ltas_power(buf[:, :4096], lens), None, buf, lens, 4096, frames=RAGGED_FRAMES)


# lengths around the kernel's 16-frame chunks at L = 4096 (31 frames: two chunks): full, one frame in the second chunk,
# an empty second chunk, a zero-padded frame, an empty clip
RAGGED = (4096, 2304, 2303, 100, 0)
RAGGED_FRAMES = (31, 17, 16, 1, 1)


def _score_views(on):
    """two logit tensors as a pitched and a transposed view, masked entries NaN"""
    xa, nf = score_case(0)
    xb, _ = score_case(1)
    B, T = xa.shape
    pit = on(torch.full((B, T + 3), float('nan')))
    pit[:, :T] = on(xa)
    tr = on(torch.full((T, B), float('nan')))
    tr.copy_(on(xb).t())
    return (pit[:, :T], tr.t()), (xa, xb), nf


def test_score_model_against_float64():
    (va, vb), (xa, xb), nf = _score_views(lambda t: t)
    acc = torch.zeros(6, dtype=torch.float64)
    eval_model.score_accum(va, nf, 0.9, True, acc)
    eval_model.score_accum(vb, nf, 0.0, False, acc)
    want = score_accum64(xa.numpy(), nf.numpy(), 0.9, True) + score_accum64(xb.numpy(), nf.numpy(), 0.0, False)
    assert want[0] == 10 and want[2] == 2 * (7 + 1 + 3 + 7 + 2)
    check_scores(acc, want)


def test_run_on_toy_networks(monkeypatch, tmp_path):
    _models(monkeypatch)
    import audiogan_amd as A
    s = _setup(A, torch.device('cpu'), 'toy', tmp_path, 4)
    _run_checks(s, tmp_path)


def test_run_moves_no_generator_and_no_loader(monkeypatch, tmp_path):
    """the training loader's next minibatch is the same whether or not an evaluation ran before it (the loader draws from
    the global numpy generator, whose state is compared too), and so is torch's next draw"""
    _models(monkeypatch)
    import audiogan_amd as A
    nxt = []
    for evaluate in (False, True):
        s = _setup(A, torch.device('cpu'), 'toy', tmp_path, 4)
        torch.manual_seed(3)
        first = next(s.loader)
        if evaluate:
            ev = _evaluator(s)
            before = (torch.random.get_rng_state(), np.random.get_state())
            ev.run()
            after = (torch.random.get_rng_state(), np.random.get_state())
            assert torch.equal(before[0], after[0]) and np.array_equal(before[1][1], after[1][1]) and before[1][2:] == after[1][2:]
        nxt.append((first, next(s.loader), torch.randn(3)))
    for a, b in zip(nxt[0][:2], nxt[1][:2]):
        assert a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[5], b[5])
    assert torch.equal(nxt[0][2], nxt[1][2])


def _record_calls(monkeypatch):
    import audiogan_amd.kernels as K
    calls = []

    def wrap(name, fn):
        def rec(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return rec
    for n in set(kernel_model.ALL) | set(eval_model.ALL):
        f = getattr(K, n)
        if callable(f) and not isinstance(f, type) and not n.endswith('_ok'):      # (launches, not the dispatch predicates)
            monkeypatch.setattr(K, n, wrap(n, f))
    return calls


def _subsequence(a, b):
    it = iter(b)
    return all(x in it for x in a)


def test_loop_with_evaluator_changes_no_training_bit(monkeypatch, tmp_path):
    """TrainLoop(evaluator=..., eval_every=2) against the same loop without one: every parameter and optimiser state bit
    equal after 4 passes; without an evaluator the loop calls ``kernels.*`` exactly as a loop built without the two
    arguments does, and the loop with one issues that sequence (weight materialisations aside) plus the evaluation's calls"""
    _models(monkeypatch)
    import audiogan_amd as A
    calls = _record_calls(monkeypatch)
    runs = []
    for mode in ('plain', 'none', 'eval'):
        s = _setup(A, torch.device('cpu'), 'toy', tmp_path, 4)
        torch.manual_seed(7)
        calls[:] = []
        kw = dict(plain={}, none=dict(evaluator=None, eval_every=2), eval=dict(eval_every=2))[mode]
        if mode == 'eval':
            kw['evaluator'] = _evaluator(s)
        lp = s.mk(fixed_critic_iter=2, gencatchup=1, stop='never', checkpoint_every=0, **kw)
        for _ in range(4):
            lp.outer()
        runs.append((lp, s, list(calls)))
    (lp0, s0, c0), (lp1, s1, c1), (lp2, s2, c2) = runs
    assert c0 == c1 and len(c0) > 100 and not set(c0) & set(eval_model.ALL)
    assert lp0.eval_log == lp1.eval_log == [] and lp0.log == lp1.log == lp2.log
    assert [(r['gen_iter'], r['dis_iter']) for r in lp2.eval_log] == [(2, 4), (4, 8)]
    assert lp2.eval_log[0] != lp2.eval_log[1]
    n = collections.Counter(c2)
    assert n['score_accum'] == 2 * 2 * 2 and n['ltas_power'] == 2 + 2 * 2
    # (the evaluation re-materialises the weights it uses: the generator's next materialisation, which the following critic
    # iteration would have issued, finds them current - the same bits, one launch moved; every other call stays in place)
    wn = lambda c: [x for x in c if x != 'weight_norm_fwd']          # noqa: E731
    assert not collections.Counter(wn(c0)) - n and _subsequence(wn(c0), wn(c2))
    for m0, m2 in zip(s0.mods, s2.mods):
        for (k, a), (_, b) in zip(m0.state_dict().items(), m2.state_dict().items()):
            assert torch.equal(a, b), k
    for o0, o2 in ((lp0.opt_g, lp2.opt_g), (lp0.opt_d, lp2.opt_d)):
        a, b = o0.state_dict(), o2.state_dict()
        assert a['step'] == b['step'] and all(torch.equal(x, y) for x, y in zip(a['s1'], b['s1']))
    assert all(torch.equal(p.grad, q.grad) for m0, m2 in zip(s0.mods, s2.mods) for p, q in zip(m0.parameters(), m2.parameters())
               if p.grad is not None)


def _ema_case(A, s):
    """two eager passes with an EMA, then an evaluation inside ``ema.applied()``: the fakes are those of the averaged weights
    (fresh modules that loaded them give the same waves) and the raw parameters keep their bits"""
    from audiogan_amd import optim
    ema = optim.EMA(s.opt_g, decay=0.5, warmup=False)
    lp = s.mk(fixed_critic_iter=2, gencatchup=1, stop='never', checkpoint_every=0, check=False, host=False, ema=ema)
    for _ in range(2):
        lp.outer()
    raw = [p.detach().clone() for m in s.mods for p in m.parameters()]
    res, parts = _evaluator(s, ema=ema).run(parts=True)
    assert all(torch.equal(p.detach(), q) for p, q in zip([p for m in s.mods for p in m.parameters()], raw))
    g2, _, e2, _ = _fresh(A, s.cfg, s.dev)
    g2.load_state_dict(ema.module_state_dict(s.mods[0]), strict=True)
    e2.load_state_dict(ema.module_state_dict(s.mods[2]), strict=True)
    res2, parts2 = _evaluator(s, mods=(g2, s.mods[1], e2, s.mods[3])).run(parts=True)
    res3, parts3 = _evaluator(s).run(parts=True)          # the last iterate
    for a, b in zip(parts, parts2):
        assert torch.equal(a['length'], b['length']) and torch.allclose(a['wave'], b['wave'], rtol=1e-5, atol=1e-6)
    for k in FLOATS:
        assert _rel(res[k], res2[k]) <= 1e-5, (k, res[k], res2[k])
    assert any(a['wave'].shape != b['wave'].shape or not torch.allclose(a['wave'], b['wave'], rtol=1e-3, atol=1e-5)
               for a, b in zip(parts, parts3))
    assert all(torch.equal(p.detach(), q) for p, q in zip([p for m in s.mods for p in m.parameters()], raw))


def test_ema_evaluation(monkeypatch, tmp_path):
    from tests import ema_model
    _models(monkeypatch)
    ema_model.install(monkeypatch)
    import audiogan_amd as A
    s = _setup(A, torch.device('cpu'), 'toy', tmp_path, 4)
    torch.manual_seed(7)
    _ema_case(A, s)


# ------------------------------------------------------------------------------------------------------------------
# GPU: the HIP kernels
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    return K_


@pytest.mark.gpu
@pytest.mark.parametrize('kind', LTAS_KINDS)
def test_ltas_power_against_float64(K, kind):
    buf, lens = ltas_case(kind)
    x, ln = buf.cuda()[:, :LTAS_L], lens.cuda()
    assert x.stride(0) == 1031
    nf = torch.full((len(lens),), -1, dtype=torch.int32, device='cuda')
    P = K.ltas_power(x, ln, nframes=nf)
    check_ltas(P, nf, buf, lens, LTAS_L, frames=LTAS_FRAMES)
    assert torch.equal(P, K.ltas_power(x, ln))
    with pytest.raises(RuntimeError):
        K.ltas_power(x.cpu(), ln)
    with pytest.raises(TypeError):
        K.ltas_power(x.double(), ln)


@pytest.mark.gpu
def test_ltas_power_long_and_ragged_clips(K):
    """more than 16 frames: the clip's frames are spread over workgroups and added by the second launch"""
    buf, lens = ltas_case('randn', L=40000, ld=40000, lens=(40000,))
    P = K.ltas_power(buf.cuda(), lens.cuda())
    check_ltas(P, None, buf, lens, 40000, frames=(311,))
    assert torch.equal(P, K.ltas_power(buf.cuda(), lens.cuda()))
    buf, lens = ltas_case('randn', L=4096, ld=4099, lens=RAGGED)
    nf = torch.full((len(lens),), -1, dtype=torch.int32, device='cuda')
    x = buf.cuda()[:, :4096]
    P = K.ltas_power(x, lens.cuda(), nframes=nf)
    check_ltas(P, nf, buf, lens, 4096, frames=RAGGED_FRAMES)
    assert float(P[4].abs().max()) == 0.0 and torch.equal(P, K.ltas_power(x, lens.cuda()))


@pytest.mark.gpu
def test_score_accum_against_float64(K):
    (va, vb), (xa, xb), nf = _score_views(lambda t: t.cuda())
    assert va.stride() == (10, 1) and vb.stride() == (1, 5)
    want = score_accum64(xa.numpy(), nf.numpy(), 0.9, True) + score_accum64(xb.numpy(), nf.numpy(), 0.0, False)
    accs = []
    for _ in range(2):
        buf = torch.zeros(8, dtype=torch.float64, device='cuda')
        buf[6:] = 123.0
        K.score_accum(va, nf.cuda(), 0.9, True, buf[:6])
        K.score_accum(vb, nf.cuda(), 0.0, False, buf[:6])
        check_scores(buf[:6], want)
        assert buf[6:].tolist() == [123.0, 123.0]
        accs.append(buf)
    assert torch.equal(accs[0], accs[1])
    with pytest.raises(TypeError):
        K.score_accum(va, nf.cuda(), 0.9, True, torch.zeros(6, device='cuda'))


@pytest.mark.gpu
@pytest.mark.parametrize('cfg', ['toy_gpu', 'c2'])
def test_run_gpu(K, tmp_path, cfg):
    import audiogan_amd as A
    K.lstm_persist_status(reset=True)
    s = _setup(A, torch.device('cuda'), cfg, tmp_path, 8)
    _run_checks(s, tmp_path)
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize('bf16', [False, True])
def test_graphed_loop_evaluates_current_weights_and_changes_no_training_bit(K, tmp_path, bf16):
    """TrainLoop(graphed=True, evaluator=..., eval_every=2) against the same loop without one, 4 passes at the C2 widths: the
    same parameter bits and the same CUDA generator state; and every recorded evaluation is what Evaluator.run gives on
    FRESH modules that loaded that iteration's state_dicts.  The loop evaluates behind a generator replay, which has just
    re-materialised the critic's weights inside itself; the hazard of the cache rule is an evaluation behind a CRITIC
    replay, whose graph materialises the critic's weights BEFORE its optimiser step and bumps no version: a fourth
    evaluation is therefore run by hand after two more critic replays (without the epoch bump and the forced refresh it
    reads weights - on bf16 storage also bfloat16 images - one step old and this comparison fails).  Float fields agree at
    1e-5 relative; in bf16 mode (storage on) at the declared elementwise tolerance of tests/test_bf16.py, 1e-2."""
    import audiogan_amd as A
    dev = torch.device('cuda')
    B = 8
    old = K.set_precision('bf16') if bf16 else None
    try:
        K.lstm_persist_status(reset=True)
        got, recs = [], []
        for evaluating in (False, True):
            s = _setup(A, dev, 'c2', tmp_path, B)
            assert s.mods[1].stores_bf16(B, dev) == bf16
            torch.cuda.manual_seed(17)
            kw = {}
            if evaluating:
                def cb(res, s=s):
                    recs.append((dict(res), [{k: v.clone() for k, v in m.state_dict().items()} for m in s.mods]))
                ev = _evaluator(s, on_eval=cb)
                kw = dict(evaluator=ev, eval_every=2)
            lp = s.mk(fixed_critic_iter=2, gencatchup=1, stop='never', checkpoint_every=0, check=False, graphed=True,
                      host=False, **kw)
            for _ in range(4):
                lp.outer()
            assert lp.gen_iter == 6 and lp._graphs is not None
            got.append(([p.detach().clone() for m in s.mods for p in m.parameters()], torch.cuda.get_rng_state()))
        lp.d_iteration()
        lp.d_iteration()
        ev.run(gen_iter=lp.gen_iter, dis_iter=lp.dis_iter)          # (behind a critic replay; recorded by the callback)
        torch.cuda.synchronize()
        assert K.lstm_persist_status() == 0
        for a, b in zip(got[0][0], got[1][0]):
            assert torch.equal(a, b)
        assert torch.equal(got[0][1], got[1][1])
        assert [r['gen_iter'] for r, _ in recs] == [2, 4, 6, 6] and [r for r, _ in recs[:3]] == lp.eval_log
        assert [r['dis_iter'] for r, _ in recs] == [4, 8, 12, 14]
        fresh = _fresh(A, 'c2', dev)
        tol = 1e-2 if bf16 else 1e-5
        for r, sds in recs:
            for m, sd in zip(fresh, sds):
                m.load_state_dict(sd, strict=True)
            want = _evaluator(s, mods=fresh).run(gen_iter=r['gen_iter'], dis_iter=r['dis_iter'])
            print(r, want)
            assert all(r[k] == want[k] for k in INTS)
            for k in FLOATS:
                assert _rel(r[k], want[k]) <= tol, (k, r[k], want[k])
        assert recs[0][0]['loss_d'] != recs[2][0]['loss_d']
        torch.cuda.synchronize()
        assert K.lstm_persist_status() == 0
    finally:
        if old is not None:
            K.set_precision(old)


@pytest.mark.gpu
def test_ema_evaluation_gpu(K, tmp_path):
    import audiogan_amd as A
    K.lstm_persist_status(reset=True)
    s = _setup(A, torch.device('cuda'), 'toy_gpu', tmp_path, 8)
    torch.cuda.manual_seed(17)
    _ema_case(A, s)
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0
