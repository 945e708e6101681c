"""-m gpu: the fronts' persistent launches (training forward, backward, generation; LSTM and GRU cell; fp32 and bf16-MFMA
forms) at frame sizes below the padded panel width - any multiple of 8 up to 256 at S = 1024 and up to 64 at S = 128, the
reference's default frame_size = 200 among them - against the per-frame path, against Generator.forward and against the
oracle.  Every case first ASSERTS that the shape takes the persistent launches."""
import collections
import os
import types

import numpy as np
import pytest
import torch

from oracle import audiogan_oracle as O
from tests.test_gpu_generate import GEN_LAG, _early_exit, _front, close

pytestmark = pytest.mark.gpu

SHAPES = [(128, 8, 5, 3), (128, 40, 40, 6), (128, 56, 64, 2), (1024, 200, 64, 4), (1024, 200, 33, 3), (1024, 104, 1, 2)]


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    assert K_.gfront_gen_persist.__module__ == 'audiogan_amd.kernels', 'real kernels must be in place'
    return K_


def _takes_persistent(K, B, S, fs):
    assert K.lib.ag_gfront_persist_ok(B, S, fs, 256) and K.lib.ag_gfront_bwd_persist_ok(B, S, fs, 256), (B, S, fs)
    dev = torch.device('cuda', 0)
    assert K.gfront_persist_ok(B, S, fs, dev) and K.gfront_bwd_persist_ok(B, S, fs, dev), (B, S, fs)


@pytest.mark.parametrize('gru', [False, True])
@pytest.mark.parametrize('S,fs,B,T', SHAPES)
def test_front_persistent_vs_per_frame(K, monkeypatch, gru, S, fs, B, T):
    """ONE persistent launch each way vs one launch per operation on the same front: frames, stop logits and every parameter
    gradient, with a contiguous output and with channel 0 of a [B, 3, T*fs] slab (frames written in place, the output
    gradient handed back as a row-pitched view).  The slab's other two channels stay zero: no store lands past column fs
    of a frame or past a row."""
    from audiogan_amd import ops, recurrent
    _takes_persistent(K, B, S, fs)
    K.lstm_persist_status(reset=True)
    front = _front(gru, S, fs, 24, 23)
    params = list(front.group.params())
    fn = ops.GRUFrontFn if gru else ops.GFrontFn
    gen = torch.Generator().manual_seed(24)
    zc = torch.randn(T, B, 24, generator=gen).cuda()
    gx, gs = torch.randn(B, T * fs, generator=gen).cuda(), torch.randn(B, T, generator=gen).cuda()
    gx_wide = torch.zeros(B, 3, T * fs).cuda()
    gx_wide[:, 0] = gx
    slab = torch.zeros(B, 3, T * fs).cuda()
    plain = recurrent._frames_buffer

    def into_slab(front_, B_, n, dev):
        assert (B_, n) == (B, T * fs)
        return slab[:, 0, :]

    # (both directions must really go through the one-launch form: count the launches' wrappers)
    calls = collections.Counter()
    for name in ('gfront_fwd_persist', 'grufront_fwd_persist', 'gfront_bwd_persist', 'grufront_bwd_persist'):
        monkeypatch.setattr(K, name, lambda *a_, _o=getattr(K, name), _n=name, **k_: (calls.update([_n]), _o(*a_, **k_))[1])
    want = {'grufront_fwd_persist': 1, 'grufront_bwd_persist': 1} if gru else {'gfront_fwd_persist': 1, 'gfront_bwd_persist': 1}
    outs = []
    old = K.PERSIST[0]
    try:
        for persist, wide in ((False, False), (True, False), (True, True)):
            K.PERSIST[0] = persist
            monkeypatch.setattr(recurrent, '_frames_buffer', into_slab if wide else plain)
            calls.clear()
            for q in params:
                q.grad = None
            x, s = fn.apply(zc, front, *params)
            assert x.stride(0) == (3 if wide else 1) * T * fs
            if wide:
                x.backward(gx_wide[:, 0], retain_graph=True)
                (s * gs).sum().backward()
            else:
                ((x * gx).sum() + (s * gs).sum()).backward()
            torch.cuda.synchronize()
            assert K.lstm_persist_status() == 0
            # (the slab pass calls backward twice, once per output: two backward launches)
            assert dict(calls) == ({k: v * (2 if wide and 'bwd' in k else 1) for k, v in want.items()} if persist else {}), dict(calls)
            outs.append((x.detach().clone(), s.detach().clone(), [q.grad.clone() for q in params]))
    finally:
        K.PERSIST[0] = old
        monkeypatch.setattr(recurrent, '_frames_buffer', plain)
    for k in (1, 2):
        close(outs[k][0], outs[0][0], rtol=1e-4, atol=1e-6, msg='frames')
        close(outs[k][1], outs[0][1], rtol=1e-4, atol=1e-5, msg='stop logits')
        for a, b in zip(outs[k][2], outs[0][2]):
            close(a, b, rtol=1e-3, atol=1e-5 * max(1.0, float(b.abs().max())), msg='gradient')
    assert torch.equal(outs[2][0], outs[1][0]) and torch.equal(outs[2][1], outs[1][1])
    assert torch.equal(slab[:, 0], outs[1][0])
    assert not bool(slab[:, 1:].any()), 'a store landed outside the frames'
    assert not bool(gx_wide[:, 1:].any()) and torch.equal(gx_wide[:, 0], gx)


@pytest.mark.parametrize('gru', [False, True])
@pytest.mark.parametrize('S,fs,B,T', SHAPES)
def test_front_backward_launch_alone(K, gru, S, fs, B, T):
    """the backward launch on synthetic saved tensors (nothing muted, no timeout set) vs the per-frame backward of the same
    tensors: dgs (LSTM) / dgi and dgh (GRU) and dxt; dxt is a view into a larger buffer whose remainder stays untouched"""
    from audiogan_amd import recurrent
    _takes_persistent(K, B, S, fs)
    ng = 3 if gru else 4
    gen = torch.Generator().manual_seed(9)
    r = lambda *shape: torch.randn(*shape, generator=gen).cuda()      # noqa: E731
    gates = torch.sigmoid(r(T, B, ng * S))
    gates[:, :, 2 * S:3 * S] = torch.tanh(r(T, B, S))
    state, gh, x = r(T + 1, B, S) * 0.5, r(T, B, ng * S) * 0.5, torch.tanh(r(B, T * fs))
    dh_ext = r(T, B, S) * 0.1
    wide = torch.zeros(B, 2, T * fs).cuda()
    wide[:, 1] = r(B, T * fs) * 0.1
    dx_ext = wide[:, 1]                                              # a row-pitched view, as the trunk's gradient slab
    whh, wih, wp = r(ng * S, S) * 0.1, r(ng * S, fs + 8) * 0.1, r(fs, S) * 0.1
    wx = wih[:, :fs]
    pad, n = 64, T * B * fs
    big = torch.full((n + 2 * pad,), 7.0).cuda()
    dxt = big[pad:pad + n].view(T, B, fs)
    dgs, dgh = torch.empty(T, B, ng * S).cuda(), torch.empty(T, B, ng * S).cuda()
    K.lstm_persist_status(reset=True)
    if gru:
        K.grufront_bwd_persist(gates, state, gh, x, dh_ext, dx_ext, whh, wx, wp, dgs, dgh, dxt)
    else:
        K.gfront_bwd_persist(gates, state, x, dh_ext, dx_ext, whh, wx, wp, dgs, dxt)
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0
    assert bool((big[:pad] == 7.0).all()) and bool((big[pad + n:] == 7.0).all()), 'a store landed outside dxt'
    # the per-frame chain, one launch per operation (GFrontFn._bwd_frames / the loop of GRUFrontFn.backward)
    rdxt = torch.empty(T, B, fs).cuda()
    if gru:
        dxa = dx_ext.contiguous().clone()
        dha = torch.zeros(T + 1, B, S).cuda()
        dha[1:] = dh_ext
        rdgi, rdgh, dh_dir = torch.empty(T, B, 3 * S).cuda(), torch.empty(T, B, 3 * S).cuda(), torch.empty(B, S).cuda()
        for t in reversed(range(T)):
            K.act_bwd2d(dxa[:, t * fs:(t + 1) * fs], x[:, t * fs:(t + 1) * fs], rdxt[t], K.ACT_TANH)
            recurrent._small_acc(rdxt[t], wp, dha[t + 1])
            K.gru_cell_bwd(gates[t], gh[t], state[t], dha[t + 1], rdgi[t], rdgh[t], dh_dir)
            K.axpby(dh_dir, dha[t], 1.0, 1.0)
            recurrent._small_acc(rdgh[t], whh, dha[t])
            if t > 0:
                recurrent._small_acc(rdgi[t], wx, dxa[:, (t - 1) * fs:t * fs])
        pairs = [(dgs, rdgi, 'dgi'), (dgh, rdgh, 'dgh'), (dxt, rdxt, 'dxt')]
    else:
        # (GFrontFn._bwd_frames takes dL/dh_t only as the stop head's rank-1 product; the same chain of launches here, with
        # a general dh_ext as the accumulator's initial value)
        dxa = dx_ext.contiguous().clone()
        dha = dh_ext.clone()
        rdgs = torch.empty(T, B, 4 * S).cuda()
        dcs = [torch.zeros(B, S).cuda(), torch.empty(B, S).cuda()]
        for t in reversed(range(T)):
            K.act_bwd2d(dxa[:, t * fs:(t + 1) * fs], x[:, t * fs:(t + 1) * fs], rdxt[t], K.ACT_TANH)
            recurrent._small_acc(rdxt[t], wp, dha[t])
            K.lstm_cell_bwd(gates[t], state[t], state[t + 1], dha[t], None, dcs[(t + 1) & 1] if t < T - 1 else None,
                            rdgs[t], dcs[t & 1])
            if t > 0:
                recurrent._small_acc(rdgs[t], whh, dha[t - 1])
                recurrent._small_acc(rdgs[t], wx, dxa[:, (t - 1) * fs:t * fs])
        pairs = [(dgs, rdgs, 'dgs'), (dxt, rdxt, 'dxt')]
    torch.cuda.synchronize()
    for a, b, name in pairs:
        close(a, b, rtol=1e-3, atol=1e-5 * max(1.0, float(b.abs().max())), msg=name)


@pytest.mark.parametrize('gru', [False, True])
@pytest.mark.parametrize('S,fs,B,T', SHAPES)
def test_generation_launch_matches_training_front(K, gru, S, fs, B, T):
    """u = 1 (no clip ever stops): the generation launch's frames and stop logits are those of the training front's
    persistent forward over all T frames; every frame runs and first = T"""
    from audiogan_amd import ops
    from audiogan_amd.recurrent import front_sample
    _takes_persistent(K, B, S, fs)
    K.lstm_persist_status(reset=True)
    front = _front(gru, S, fs, 24, 31)
    zc = torch.randn(T, B, 24, generator=torch.Generator().manual_seed(37)).cuda()
    with torch.no_grad():
        fn = ops.GRUFrontFn if gru else ops.GFrontFn
        x_ref, s_ref = fn.apply(zc, front, *front.group.params())
        x, s, first, t_run = front_sample(front, zc, torch.ones(T, B, device='cuda'))
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0
    assert t_run is not None, 'the generation launch did not run'
    close(x, x_ref, rtol=1e-4, atol=1e-6, msg='frames')
    close(s, s_ref, rtol=1e-4, msg='stop logits')
    assert int(t_run) == T and bool((first == T).all())


@pytest.mark.parametrize('gru', [False, True])
@pytest.mark.parametrize('S,fs', [(1024, 200), (128, 40)])
@pytest.mark.parametrize('B', [1, 33, 64])
def test_generate_exits_early_and_matches_forward(K, gru, S, fs, B):
    """Generator.generate with stops drawn at known frames (the last at frame 5 of 32): length = (frames + 1) * fs, the loop
    ran 6 .. 6 + GEN_LAG frames (last_t_run: the launch, not the per-frame fallback), wave and logits are Generator.forward's
    given the same stop draws"""
    _takes_persistent(K, B, S, fs)
    assert GEN_LAG == 1
    _early_exit(K, gru, S, fs, B)


def test_generate_bf16_mode_at_the_default_frame_size(K):
    """AG_PREC_BF16 (the bf16-MFMA form of the front, PM = 2) at frame 200: the early-exit case against the bf16 forward"""
    from tests.test_bf16 import close_bf16
    _takes_persistent(K, 64, 1024, 200)
    old = K.set_precision('bf16')
    try:
        _early_exit(K, False, 1024, 200, 64, tol=lambda a, b, m: close_bf16(a, b, m))
    finally:
        K.set_precision(old)


def test_bf16_mfma_front_vs_rounded_oracle_at_the_default_frame_size(K):
    """the S = 1024 generator front at frame 200 on the bf16-MFMA forms of the persistent launches vs the bf16-rounded
    oracle: generated frames and all gradients (the generator half of test_bf16_mfma_persistent_recurrent_kernels)"""
    import audiogan_amd as A
    from tests.test_bf16 import close_bf16
    B, T, fs = 40, 3, 200
    _takes_persistent(K, B, 1024, fs)
    gcfg = dict(frame_size=fs, embed_size=8, noise_size=8, state_size=1024, num_layers=1, struct=[[9, 4, 8, 4]])
    torch.manual_seed(41)
    go = O.Generator(**gcfg)
    g = A.Generator(**gcfg)
    g.load_state_dict(go.state_dict())
    g.cuda()
    gen = torch.Generator().manual_seed(42)
    c, z = torch.randn(B, 8, generator=gen), torch.randn(B, T, 8, generator=gen)
    wx = torch.randn(B, T * fs, generator=gen)
    old = K.set_precision('bf16')
    try:
        K.lstm_persist_status(reset=True)
        with O.bf16_mode():
            xo = go(z=z, c=c, stop=torch.zeros(B, T, dtype=torch.long))[0]
            (xo * wx).sum().backward()
        xg = g(z=z.cuda(), c=c.cuda(), stop='never')[0]
        (xg * wx.cuda()).sum().backward()
        torch.cuda.synchronize()
    finally:
        K.set_precision(old)
    assert K.lstm_persist_status() == 0
    close_bf16(xg, xo, 'waveform')
    rp = dict(go.named_parameters())
    for k, q in g.named_parameters():
        if (k.split('.')[-1].startswith('bias') and k.endswith('_v')) or rp[k].grad is None:
            continue
        close_bf16(q.grad, rp[k].grad, k, elem=5e-2, l2=5e-2 if k.endswith('_g') else 2e-2)


def test_reference_defaults_small_batch_vs_oracle(K):
    """the reference's default widths end to end (audiogan.py:557: frame 200, state 1024, default structs): G and the ragged
    D, B = 2, T = 41 frames = 8200 samples (what the loader makes of an 8192-sample clip on the frame grid), critic lengths
    [8200, 5000]; outputs, activations, logits and all gradients vs the oracle with the same weights.  Both conv stacks run at
    a length that is not a power of two."""
    import audiogan_amd as A
    from tests.test_gpu_modules import _grads_close
    from tests.test_gpu_modules import close as mclose
    fs, B, T = 200, 2, 41
    _takes_persistent(K, B, 1024, fs)
    torch.manual_seed(0)
    go = O.Generator(frame_size=fs, embed_size=100, noise_size=100, state_size=1024)
    do = O.Discriminator(state_size=1024, embed_size=100)
    g = A.Generator(frame_size=fs, embed_size=100, noise_size=100, state_size=1024)
    d = A.Discriminator(state_size=1024, embed_size=100)
    g.load_state_dict(go.state_dict()); d.load_state_dict(do.state_dict())
    g.cuda(); d.cuda()
    assert g.front_is_persistent(B, torch.device('cuda', 0))
    K.lstm_persist_status(reset=True)
    gen = torch.Generator().manual_seed(1)
    z, c = torch.randn(B, T, 100, generator=gen), torch.randn(B, 100, generator=gen)
    stop = torch.zeros(B, T, dtype=torch.long)
    xo, so, _, lo = go(z=z, c=c, stop=stop)
    x, s, _, l = g(z=z.cuda(), c=c.cuda(), stop='never')
    assert tuple(x.shape) == (B, T * fs) and torch.equal(l.cpu(), lo)
    mclose(x, xo); mclose(s, so)
    lens = torch.tensor([T * fs, 5000])
    lgo, actso, _, nfo = do(xo.detach(), lens, c)
    lg, acts, _, nf = d(x.detach(), lens.cuda(), c.cuda())
    np.testing.assert_array_equal(nf.cpu().numpy(), nfo.numpy())
    for a, b in zip(acts, actso):
        mclose(a, b)
    mclose(lg, lgo, scale_atol=1e-4)
    # backward through D into G
    w = torch.randn(lgo.shape, generator=gen)
    xo2, _, _, _ = go(z=z, c=c, stop=stop)
    (do(xo2, lens, c)[0] * w).sum().backward()
    x2, _, _, _ = g(z=z.cuda(), c=c.cuda(), stop='never')
    (d(x2, lens.cuda(), c.cuda())[0] * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0
    _grads_close(d, {k: p.grad for k, p in do.named_parameters()}, scale_atol=1e-3)
    _grads_close(g, {k: (p.grad if p.grad is not None else torch.zeros_like(p))
                     for k, p in go.named_parameters()}, scale_atol=1e-3)


def _loop_setup(A, dev, tmp_path, B):
    """tests.test_loop._setup at small widths with a frame size only the padded panel accepts: S = 128, fs = 40"""
    from audiogan_amd import dataset as D
    from audiogan_amd import loop, optim
    torch.manual_seed(81)
    frame, maxlen = 40, 320
    gcfg = dict(frame_size=frame, embed_size=8, noise_size=8, state_size=128, num_layers=1, struct=[[17, 8, 16, 8], [9, 4, 16, 8]])
    dcfg = dict(state_size=64, embed_size=8, num_layers=1, cnn_struct=[[7, 2, 8], [7, 2, 16]])
    ecfg = dict(output_size=8, char_embed_size=6, num_chars=256)
    g, d = A.Generator(**gcfg).to(dev), A.Discriminator(**dcfg).to(dev)
    e_g, e_d = A.Embedder(**ecfg).to(dev), A.Embedder(**ecfg).to(dev)
    opt_g = optim.make_optimizer(list(g.parameters()) + list(e_g.parameters()), 'rmsprop', 1e-4)
    opt_d = optim.make_optimizer(list(d.parameters()) + list(e_d.parameters()), 'rmsprop', 1e-4)
    words = ['alpha', 'beta', 'gamma', 'delta', 'epsil', 'zetaa', 'etaaa', 'theta', 'iotaa', 'kappa', 'lambd']
    ds = D.SyntheticWordDataset(words, n_per_word=3, min_len=maxlen // 3, max_len=maxlen, kind='noise', seed=3)
    args = types.SimpleNamespace(conditional=True, dataset=ds, minwordlen=1, subset=None, amplitudes=0)
    np.random.seed(5)
    h5, ml, gen_train, _, keys_train, _ = D.dataloader(B, args, maxlen=maxlen, frame_size=frame)
    pick = loop.words_picker(D, B, ml, h5, keys_train, args, frame_size=frame)
    prefix = os.path.join(tmp_path, 'run')
    mk = lambda **kw: loop.TrainLoop(g, d, e_g, e_d, opt_g, opt_d, gen_train, pick, B, ml, dev, checkpoint_prefix=prefix, **kw)  # noqa: E731
    return mk, (g, d, e_g, e_d)


def test_captured_iterations_replay_the_eager_loop_bit_for_bit(K, tmp_path):
    """TrainLoop(graphed=True) at S = 128, fs = 40 (a frame size the fronts' persistent launches newly accept), stop='never':
    the captured iterations leave the same bits in every parameter as the Python-issued loop (host=False) on the same loader
    batches and the same device random stream"""
    import audiogan_amd as A
    dev = torch.device('cuda')
    B = 8
    _takes_persistent(K, B, 128, 40)
    K.lstm_persist_status(reset=True)
    got = []
    for graphed in (False, True):
        mk, mods = _loop_setup(A, dev, tmp_path, B)
        assert mods[0].front_is_persistent(B, dev)
        torch.cuda.manual_seed(17)
        lp = mk(fixed_critic_iter=2, gencatchup=1, stop='never', checkpoint_every=0, check=False, graphed=graphed, host=False)
        for _ in range(4 if graphed else 6):
            ran, rd, rg = lp.outer()
        assert lp.dis_iter == 12 and lp.gen_iter == 6
        if graphed:
            assert lp._graphs is not None and set(lp._graphs) == {'d0', 'd1', 'g'}
        got.append(([p.detach().clone() for m in mods for p in m.parameters()],
                    [float(rd['loss']), float(rd['acc_d']), float(rd['acc_g']), float(rg['loss']), float(rg['baseline'])]))
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0
    assert got[0][1] == got[1][1], (got[0][1], got[1][1])
    assert all(np.isfinite(v) for v in got[0][1])
    for p, q in zip(got[0][0], got[1][0]):
        assert torch.equal(p, q)
    mk, mods = _loop_setup(A, dev, tmp_path, B)
    moved = sum(int(not torch.equal(p, q.detach())) for p, q in zip(got[0][0], [p for m in mods for p in m.parameters()]))
    assert moved > 0.9 * len(got[0][0])          # (and the passes did train: nearly every tensor left its initial value)
