"""-m gpu: the generation mode of the fronts' persistent launch (ag_gfront_fwd, gen = 1) and Generator.generate on the HIP
kernels - against the training front, against Generator.forward given the same stop draws, on the per-frame fallback, in
bf16 mode and between the replays of a graphed TrainLoop."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GEN_LAG = 1      # csrc/front_parts.h


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    assert K_.gfront_gen_persist.__module__ == 'audiogan_amd.kernels', 'real kernels must be in place'
    return K_


def close(got, ref, rtol=1e-4, atol=None, msg=''):
    ref, got = ref.detach().cpu().float().numpy(), got.detach().cpu().float().numpy()
    if atol is None:
        atol = 1e-5 * max(1.0, float(np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol, err_msg=msg)


def _front(gru, S, fs, Fz, seed):
    from audiogan_amd import ops
    gen = torch.Generator().manual_seed(seed)
    ng = 3 if gru else 4
    front = ops.GRUFront(fs, S) if gru else ops.GFront(fs, 1, S)
    shapes = [(ng * S, fs + Fz), (ng * S, S), (ng * S,), (ng * S,), (fs, S), (fs,), (1, S), (1,)]
    for shp in shapes:
        v = torch.nn.Parameter((torch.randn(shp, generator=gen) / (shp[-1] ** 0.5 if len(shp) > 1 else 4.0)).cuda())
        gq = torch.nn.Parameter((v.detach().reshape(shp[0], -1).norm(dim=1) if len(shp) > 1 else v.detach().abs())
                                .view([shp[0]] + [1] * (len(shp) - 1)).clone())
        front.group.add(v, gq)
    return front


@pytest.mark.parametrize('gru', [False, True])
@pytest.mark.parametrize('S,fs,B,T', [(128, 64, 7, 1), (128, 64, 40, 6), (1024, 256, 64, 4), (1024, 256, 33, 3)])
def test_generation_launch_matches_training_front(K, gru, S, fs, B, T):
    """u = 1 (no clip ever stops): the generation launch's frames and stop logits are those of the training front's
    persistent forward over all T frames; every frame runs and first = T"""
    from audiogan_amd import ops
    from audiogan_amd.recurrent import front_sample
    assert K.gfront_persist_ok(B, S, fs, torch.device('cuda'))
    K.lstm_persist_status(reset=True)
    front = _front(gru, S, fs, 24, 31)
    zc = torch.randn(T, B, 24, generator=torch.Generator().manual_seed(37)).cuda()
    with torch.no_grad():
        fn = ops.GRUFrontFn if gru else ops.GFrontFn
        x_ref, s_ref = fn.apply(zc, front, *front.group.params())
        x, s, first, t_run = front_sample(front, zc, torch.ones(T, B, device='cuda'))
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0
    close(x, x_ref, rtol=1e-4, atol=1e-6, msg='frames')
    close(s, s_ref, rtol=1e-4, msg='stop logits')
    assert int(t_run) == T and bool((first == T).all())


def _generator(gru, S, fs):
    import audiogan_amd as A
    torch.manual_seed(41)
    if S == 1024:       # C2 widths (C4 for the GRU front)
        cfg = dict(frame_size=fs, embed_size=100, noise_size=100, state_size=S)
    else:
        cfg = dict(frame_size=fs, embed_size=8, noise_size=8, state_size=S, struct=[[17, 8, 16, 8], [9, 4, 16, 8]])
    g = A.GRUGenerator(**cfg) if gru else A.Generator(num_layers=1, **cfg)
    return g.cuda(), cfg['noise_size'], cfg['embed_size']


def _inputs(B, T, ns, es, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, ns, generator=gen).cuda(), torch.randn(B, es, generator=gen).cuda()


def _pattern(B, T, last=5):
    """u [T,B] = 0 at clip b's stop frame (5 - b) % 6 (clip 0 at frame `last`), 1 elsewhere; the stop draws as a [B,T] tensor"""
    frames = torch.tensor([(last - b) % (last + 1) for b in range(B)])
    u = torch.ones(T, B)
    u[frames, torch.arange(B)] = 0.0
    stops = torch.zeros(B, T, dtype=torch.long)
    stops[torch.arange(B), frames] = 1
    return u.cuda(), stops.cuda(), frames.cuda()


def _early_exit(K, gru, S, fs, B, tol=None):
    T = 32
    g, ns, es = _generator(gru, S, fs)
    z, c = _inputs(B, T, ns, es, 43)
    u, stops, frames = _pattern(B, T)
    K.lstm_persist_status(reset=True)
    wave, s, stop_list, length = g.generate(c, z=z, u=u)
    t_run = int(g.last_t_run)
    with torch.no_grad():
        wf, sf, _, lf = g(z=z, c=c, stop=stops)
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0
    assert torch.equal(length, (frames + 1) * fs) and torch.equal(lf, length)
    assert 6 <= t_run <= 6 + GEN_LAG, t_run
    assert len(stop_list) == 6 and torch.equal(torch.cat(stop_list, 1), stops[:, :6])
    if tol is None:
        close(wave, wf, rtol=1e-4, msg='wave')
        close(s, sf, rtol=1e-4, msg='stop logits')
    else:
        tol(wave, wf, 'wave')
        tol(s, sf, 'stop logits')
    return wave, length, stops


@pytest.mark.parametrize('gru', [False, True])
@pytest.mark.parametrize('S,fs', [(128, 64), (1024, 256)])
@pytest.mark.parametrize('B', [1, 33, 64])
def test_generate_exits_early_and_matches_forward(K, gru, S, fs, B):
    """stops drawn at known frames (the last at frame 5 of 32): first is exact, the loop ran at most 6 + GEN_LAG frames, and
    wave / length / logits are Generator.forward's given the same stop draws (one and two row tiles, a partial tile)"""
    _early_exit(K, gru, S, fs, B)


@pytest.mark.parametrize('gru', [False, True])
def test_generate_random_draws_match_forward(K, gru):
    S, fs, B, T = 1024, 256, 64, 32
    g, ns, es = _generator(gru, S, fs)
    z, c = _inputs(B, T, ns, es, 47)
    u = torch.rand(T, B, generator=torch.Generator(device='cuda').manual_seed(5), device='cuda')
    K.lstm_persist_status(reset=True)
    wave, s, stop_list, length = g.generate(c, z=z, u=u)
    draws = torch.cat(stop_list, 1)
    p, uu = torch.sigmoid(s), u[:s.size(1)].t()
    clear = (uu - p).abs() > 1e-5
    assert torch.equal(draws.bool()[clear], (uu < p)[clear])
    stops = torch.zeros(B, T, dtype=torch.long, device='cuda')
    stops[:, :draws.size(1)] = draws
    with torch.no_grad():
        wf, sf, _, lf = g(z=z, c=c, stop=stops)
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0
    assert torch.equal(length, lf) and int(g.last_t_run) <= min(T, s.size(1) + GEN_LAG)
    close(wave, wf, rtol=1e-4, msg='wave')
    close(s, sf, rtol=1e-4, msg='stop logits')


def test_generate_bf16_mode(K):
    """AG_PREC_BF16 (the bf16-MFMA form of the front, PM = 2): the early-exit case against the bf16 forward, at the tolerance
    of the bf16 front tests"""
    from tests.test_bf16 import close_bf16
    old = K.set_precision('bf16')
    try:
        _early_exit(K, False, 1024, 256, 64, tol=lambda a, b, m: close_bf16(a, b, m))
    finally:
        K.set_precision(old)


@pytest.mark.parametrize('gru', [False, True])
def test_generate_fallback_matches_persistent(K, gru):
    """K.PERSIST off: the per-frame front over all T frames and the same rule on its logits - the same first / length as the
    persistent launch and the same waves to tolerance"""
    S, fs, B = 1024, 256, 40
    wave, length, stops = _early_exit(K, gru, S, fs, B)
    g, ns, es = _generator(gru, S, fs)
    z, c = _inputs(B, 32, ns, es, 43)
    u, _, _ = _pattern(B, 32)
    old = K.PERSIST[0]
    K.PERSIST[0] = False
    try:
        w2, _, sl2, l2 = g.generate(c, z=z, u=u)
    finally:
        K.PERSIST[0] = old
    torch.cuda.synchronize()
    assert g.last_t_run is None and K.lstm_persist_status() == 0
    assert torch.equal(l2, length) and torch.equal(torch.cat(sl2, 1), stops[:, :6])
    close(w2, wave, rtol=1e-4, msg='wave')


def test_graphed_loop_samples_use_current_weights_and_change_no_training_bit(K, tmp_path):
    """TrainLoop(graphed=True, sample_every=2) against the same loop without sampling: the same parameter bits after the same
    passes; and every sample the callback received is what generate gives on a FRESH generator that loaded that iteration's
    state_dict, with the same z, words and u (the captured optimiser bumps no parameter version: stale weights would differ)"""
    import audiogan_amd as A
    from tests.test_loop import _setup
    dev = torch.device('cuda')
    B = 8
    words = (np.random.RandomState(0).randint(97, 123, size=(B, 5)), np.array([5, 3, 4, 2, 5, 1, 4, 3]))
    K.lstm_persist_status(reset=True)
    got, samples = [], []
    for sampling in (False, True):
        mk, mods, _ = _setup(A, dev, True, tmp_path, B)
        g, e_g = mods[0], mods[2]
        torch.cuda.manual_seed(17)
        kw = {}
        if sampling:
            def cb(n, wave, length, stop_list):
                samples.append(dict(n=n, wave=wave.clone(), length=length.clone(), u=lp.last_sample_u.clone(),
                                    g={k: v.clone() for k, v in g.state_dict().items()},
                                    e_g={k: v.clone() for k, v in e_g.state_dict().items()}))
            kw = dict(sample_every=2, sample_words=words, sample_seed=11, on_sample=cb)
        lp = mk(fixed_critic_iter=2, gencatchup=1, stop='never', checkpoint_every=0, check=False, graphed=True, host=False, **kw)
        for _ in range(4):
            lp.outer()
        assert lp.gen_iter == 6
        got.append([p.detach().clone() for m in mods for p in m.parameters()])
        if sampling:
            z = lp.sample_z.clone()
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0
    for a, b in zip(got[0], got[1]):
        assert torch.equal(a, b)
    assert [d['n'] for d in samples] == [2, 4, 6]
    g2 = A.Generator(frame_size=256, embed_size=100, noise_size=100, state_size=1024, num_layers=1).to(dev)
    e2 = A.Embedder(output_size=100, char_embed_size=50, num_layers=1, num_chars=256).to(dev)
    cs, cl = torch.from_numpy(words[0]).long().to(dev), torch.from_numpy(words[1]).long().to(dev)
    for d in samples:
        g2.load_state_dict(d['g'])
        e2.load_state_dict(d['e_g'])
        with torch.no_grad():
            w, _, _, ln = g2.generate(e2(cs, cl), z=z, u=d['u'])
        assert torch.equal(ln, d['length']), d['n']
        close(d['wave'], w, rtol=1e-5, atol=1e-6, msg='sample of generator iteration %d' % d['n'])
