"""optim.EMA: the moving average of the generator's weights (kernels.ema_update / ag_ema_update), sampling with it
(EMA.applied, TrainLoop(ema=..., sample_ema=...)) and its checkpoints.  CPU: host logic on the kernel models
(tests/kernel_model.py + tests/ema_model.py); -m gpu: the HIP kernel, eager and captured.

The bound of one update, 5 * 2^-24 * max(|p|, |e|) per element, is three fp32 roundings: the difference p - e has magnitude
at most 2 max (2 units), the product 2 more if the compiler does not fuse it, the sum 1."""
import contextlib
import os

import numpy as np
import pytest
import torch

from tests import ema_model, kernel_model
from tests.ema_model import STEP_BOUND, lerp64, weight

GCFG = dict(frame_size=32, embed_size=8, noise_size=8, state_size=64, num_layers=1, struct=[[17, 8, 16, 8], [9, 4, 16, 8]])
DCFG = dict(state_size=64, embed_size=8, num_layers=1, cnn_struct=[[7, 2, 8], [7, 2, 16]])
ECFG = dict(output_size=8, char_embed_size=6, num_chars=256)
B = 4
WORDS = (np.random.RandomState(0).randint(97, 123, size=(B, 5)), np.array([5, 3, 4, 2]))


def _models(monkeypatch):
    kernel_model.install(monkeypatch)
    ema_model.install(monkeypatch)


def _toy(dev='cpu', seed=0):
    """three parameters under an RMSprop; the last one never receives a gradient"""
    from audiogan_amd import optim
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in ((5,), (3, 4), (1,), (7,))]
    return ps, optim.RMSprop(ps, lr=1e-2)


def _toy_step(ps, opt, gen):
    for p in ps[:-1]:
        p.grad = torch.randn(p.shape, generator=gen).to(p.device)
    opt.step()


def _within(shadow, ref64, bound, msg=''):
    err = (shadow.detach().double().reshape(-1) - ref64.reshape(-1)).abs()
    bad = err > bound.reshape(-1)
    assert not bool(bad.any()), '%s: %d elements over the bound, worst %.3g x' % (
        msg, int(bad.sum()), float((err / bound.reshape(-1).clamp_min(1e-300)).max()))


# ------------------------------------------------------------------------------------------------------------------
# CPU: kernel model + ema model
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('warmup', [True, False])
def test_formula_and_warmup(monkeypatch, warmup):
    _models(monkeypatch)
    from audiogan_amd import optim
    ps, opt = _toy()
    gen = torch.Generator().manual_seed(1)
    ema = optim.EMA(opt, decay=0.999, warmup=warmup)
    assert ema.step0 == 0 and all(torch.equal(s, p.detach().reshape(-1)) for s, p in zip(ema.shadows, ps))
    assert all(s.data_ptr() % 16 == 0 for s in ema.shadows)
    frozen = ps[-1].detach().clone()
    ref = [p.detach().double().reshape(-1) for p in ps]
    mx = [r.abs() for r in ref]
    for k in range(1, 13):
        _toy_step(ps, opt, gen)
        ema.update()
        w = weight(0.999, warmup, k)
        if k == 1:
            assert w == (np.float32(1) - np.float32(2) / np.float32(11) if warmup else np.float32(1) - np.float32(0.999))
        for i, p in enumerate(ps):
            mx[i] = torch.maximum(torch.maximum(mx[i], ref[i].abs()), p.detach().double().reshape(-1).abs())
            ref[i] = lerp64(ref[i], p.reshape(-1), w)
            _within(ema.shadows[i], ref[i], k * STEP_BOUND * mx[i], 'step %d tensor %d' % (k, i))
    # a parameter whose .grad stays None: the average is the parameter, bit for bit
    assert ps[-1].grad is None and torch.equal(ps[-1].detach(), frozen) and torch.equal(ema.shadows[-1], frozen.reshape(-1))
    assert not torch.equal(ema.shadows[0], ps[0].detach().reshape(-1))
    # an EMA constructed after 5 optimiser steps: its k starts at 1
    ps, opt = _toy(seed=3)
    for _ in range(5):
        _toy_step(ps, opt, gen)
    ema = optim.EMA(opt, decay=0.999, warmup=True)
    assert ema.step0 == 5
    e0 = [s.double().clone() for s in ema.shadows]
    _toy_step(ps, opt, gen)
    ema.update()
    for i, p in enumerate(ps[:-1]):
        want = lerp64(e0[i], p.reshape(-1), weight(0.999, True, 1))
        _within(ema.shadows[i], want, STEP_BOUND * torch.maximum(e0[i].abs(), p.detach().double().reshape(-1).abs()), 'k = 1')
        far = lerp64(e0[i], p.reshape(-1), weight(0.999, True, 6))       # (what k = 6 would have given)
        assert not torch.allclose(ema.shadows[i].double(), far, rtol=1e-4, atol=0)
    with pytest.raises(ValueError):
        optim.EMA(opt, decay=1.5)


def test_applied_restores(monkeypatch):
    _models(monkeypatch)
    from audiogan_amd import common, optim
    ps, opt = _toy()
    gen = torch.Generator().manual_seed(2)
    ema = optim.EMA(opt, decay=0.9, warmup=False)
    for _ in range(3):
        _toy_step(ps, opt, gen)
        ema.update()
    before = [p.detach().clone() for p in ps]
    ptrs = [p.data_ptr() for p in ps]
    shadows = [s.clone() for s in ema.shadows]

    def check_block(raises):
        ep0 = [common.param_epoch(p) for p in ps]
        with (pytest.raises(ZeroDivisionError) if raises else contextlib.nullcontext()):
            with ema.applied():
                assert all(torch.equal(p.detach().reshape(-1), s) for p, s in zip(ps, shadows))
                assert [p.data_ptr() for p in ps] == ptrs
                ep1 = [common.param_epoch(p) for p in ps]
                assert all(b > a for a, b in zip(ep0, ep1))
                with pytest.raises(RuntimeError):
                    with ema.applied():
                        pass
                with pytest.raises(RuntimeError):
                    ema.update()
                if raises:
                    1 / 0
        assert all(torch.equal(p.detach(), q) for p, q in zip(ps, before))
        assert [p.data_ptr() for p in ps] == ptrs
        assert all(b > a for a, b in zip(ep1, [common.param_epoch(p) for p in ps]))
        assert all(torch.equal(s, t) for s, t in zip(ema.shadows, shadows))

    assert any(not torch.equal(p.detach().reshape(-1), s) for p, s in zip(ps, shadows))
    check_block(False)
    check_block(True)
    check_block(False)          # (usable again after the exception)
    ema.update()


def _loop_run(A, tmp_path, passes, with_ema, sample_ema=True, snaps=None, **kw):
    """tests.test_loop._setup at the small widths; passes of 2 critic + 1 generator iteration from fixed seeds.  ``snaps``
    receives opt_g's parameters as they are at the start and after every generator iteration"""
    from audiogan_amd import optim
    from tests.test_loop import _setup
    mk, mods, prefix = _setup(A, torch.device('cpu'), False, tmp_path, B)
    torch.manual_seed(7)
    opt_g = mk(checkpoint_every=0).opt_g
    ema = optim.EMA(opt_g, decay=0.9, warmup=True) if with_ema else None
    on_sample = None
    if snaps is not None:
        on_sample = lambda n, *a: snaps.append([p.detach().clone() for p in opt_g.params])     # noqa: E731
        on_sample(0)
    args = dict(fixed_critic_iter=2, gencatchup=1, stop='never', checkpoint_every=0, sample_every=1, sample_words=WORDS,
                sample_seed=3, on_sample=on_sample)
    args.update(kw)
    if ema is not None:
        args.update(ema=ema, sample_ema=sample_ema)
    lp = mk(**args)
    for _ in range(passes):
        lp.outer()
    return lp, mods, ema, prefix


def test_ema_changes_no_training_bit(monkeypatch, tmp_path):
    _models(monkeypatch)
    import audiogan_amd as A
    lp0, mods0, _, _ = _loop_run(A, tmp_path, 3, False)
    snaps = []
    lp1, mods1, ema, _ = _loop_run(A, tmp_path, 3, True, snaps=snaps)
    assert lp0.log == lp1.log and lp1.gen_iter == 3 and len(snaps) == 4
    for m0, m1 in zip(mods0, mods1):
        for (k, a), (_, b) in zip(m0.state_dict().items(), m1.state_dict().items()):
            assert torch.equal(a, b), k
    for o0, o1 in ((lp0.opt_g, lp1.opt_g), (lp0.opt_d, lp1.opt_d)):
        s0, s1 = o0.state_dict(), o1.state_dict()
        assert s0['step'] == s1['step'] and all(torch.equal(a, b) for a, b in zip(s0['s1'], s1['s1']))
    # the shadows against the float64 recursion over the parameters recorded after every generator iteration
    ref = [p.double().reshape(-1) for p in snaps[0]]
    assert len(ref) == len(ema.shadows) == len(list(mods1[0].parameters())) + len(list(mods1[2].parameters()))
    mx = [r.abs() for r in ref]
    for k, snap in enumerate(snaps[1:], 1):
        for i, p in enumerate(snap):
            mx[i] = torch.maximum(mx[i], p.double().reshape(-1).abs())
            ref[i] = lerp64(ref[i], p.reshape(-1), weight(0.9, True, k))
    moved = 0
    for i, s in enumerate(ema.shadows):
        _within(s, ref[i], 3 * STEP_BOUND * mx[i], 'tensor %d' % i)
        moved += int(not torch.equal(s, snaps[-1][i].reshape(-1)))
    assert moved > 0.5 * len(ema.shadows)


@pytest.mark.parametrize('sample_ema', [True, False])
def test_samples_use_the_average(monkeypatch, tmp_path, sample_ema):
    _models(monkeypatch)
    import audiogan_amd as A
    seen = {}

    def on_sample(n, wave, length, stop_list):
        # (called outside ``applied()``: the parameters are the raw ones again)
        seen.update(n=n, wave=wave.clone(), length=length.clone(), g=dict(seen['ema'].module_state_dict(seen['mods'][0])),
                    e=dict(seen['ema'].module_state_dict(seen['mods'][2])),
                    graw={k: v.clone() for k, v in seen['mods'][0].state_dict().items()},
                    eraw={k: v.clone() for k, v in seen['mods'][2].state_dict().items()})

    from audiogan_amd import optim
    from tests.test_loop import _setup
    mk, mods, _ = _setup(A, torch.device('cpu'), False, tmp_path, B)
    torch.manual_seed(7)
    ema = optim.EMA(mk(checkpoint_every=0).opt_g, decay=0.9, warmup=False)
    seen.update(ema=ema, mods=mods)
    lp = mk(fixed_critic_iter=2, gencatchup=1, stop='never', checkpoint_every=0, sample_every=1, sample_words=WORDS,
            sample_seed=3, on_sample=on_sample, ema=ema, sample_ema=sample_ema)
    for _ in range(2):
        lp.outer()
    assert seen['n'] == 2
    g2, e2 = A.Generator(**GCFG), A.Embedder(**ECFG)
    g2.load_state_dict(seen['g'] if sample_ema else seen['graw'], strict=True)
    e2.load_state_dict(seen['e'] if sample_ema else seen['eraw'], strict=True)
    cs, cl = torch.from_numpy(WORDS[0]).long(), torch.from_numpy(WORDS[1]).long()
    with torch.no_grad():
        wave, _, _, length = g2.generate(e2(cs, cl), z=lp.sample_z, u=lp.last_sample_u)
    assert torch.equal(wave, seen['wave']) and torch.equal(length, seen['length'])
    # ... and the other set of weights gives another wave
    g2.load_state_dict(seen['graw'] if sample_ema else seen['g'], strict=True)
    e2.load_state_dict(seen['eraw'] if sample_ema else seen['e'], strict=True)
    with torch.no_grad():
        other = g2.generate(e2(cs, cl), z=lp.sample_z, u=lp.last_sample_u)[0]
    assert other.shape != wave.shape or not torch.equal(other, wave)


def test_checkpoint_round_trip(monkeypatch, tmp_path):
    _models(monkeypatch)
    import audiogan_amd as A
    from audiogan_amd import checkpoint, loop, optim
    from oracle import audiogan_oracle as O
    kw = dict(sample_every=0, sample_words=None, on_sample=None)
    lpa, _, ema_a, _ = _loop_run(A, tmp_path / 'a', 4, True, **kw)
    want = [s.clone() for s in ema_a.shadows]
    os.makedirs(tmp_path / 'b')
    lpb, mods_b, ema_b, prefix = _loop_run(A, tmp_path / 'b', 2, True, checkpoint_every=2, **kw)
    for role in ('gen', 'eg', 'genema', 'egema', 'opt'):
        assert os.path.exists('%s-%s-%05d' % (prefix, role, 2)), role
    # fresh modules (another initialisation), optimisers and EMA on the same loader: resume and go on
    torch.manual_seed(1234)
    g, d, e_g, e_d = A.Generator(**GCFG), A.Discriminator(**DCFG), A.Embedder(**ECFG), A.Embedder(**ECFG)
    opt_g = optim.make_optimizer(list(g.parameters()) + list(e_g.parameters()), 'rmsprop', 1e-4)
    opt_d = optim.make_optimizer(list(d.parameters()) + list(e_d.parameters()), 'rmsprop', 1e-4)
    ema = optim.EMA(opt_g, decay=0.5, warmup=False)
    lp = loop.TrainLoop(g, d, e_g, e_d, opt_g, opt_d, lpb.loader, lpb.pick_words, B, lpb.maxlen, 'cpu', checkpoint_prefix=prefix,
                        fixed_critic_iter=2, gencatchup=1, stop='never', checkpoint_every=2, ema=ema)
    lp.resume(2)
    assert (ema.decay, ema.warmup, ema.step0) == (0.9, True, 0) and lp.gen_iter == 2
    assert all(torch.equal(a, b) for a, b in zip(ema.shadows, ema_b.shadows))
    for _ in range(2):
        lp.outer()
    assert lp.gen_iter == 4
    for a, b in zip(ema.shadows, want):
        assert torch.equal(a, b)
    # the averaged weights as plain state_dicts: strict into this package's modules and the reference-shaped ones
    sd_g = torch.load('%s-genema-%05d' % (prefix, 4), weights_only=True)
    sd_e = torch.load('%s-egema-%05d' % (prefix, 4), weights_only=True)
    g3, e3 = A.Generator(**GCFG), A.Embedder(**ECFG)
    g3.load_state_dict(sd_g, strict=True)
    e3.load_state_dict(sd_e, strict=True)
    O.Generator(**GCFG).load_state_dict(sd_g, strict=True)
    got = [p.detach().reshape(-1) for p in list(g3.parameters()) + list(e3.parameters())]
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    assert any(not torch.equal(a, p.detach().reshape(-1)) for a, p in zip(got, ema.params))
    g4, e4 = A.Generator(**GCFG), A.Embedder(**ECFG)
    assert checkpoint.load(prefix, 4, g=g4, e_g=e4, use_ema=True)['gen_iter'] == 4
    assert all(torch.equal(p.detach().reshape(-1), b) for p, b in zip(list(g4.parameters()) + list(e4.parameters()), want))
    checkpoint.load(prefix, 4, g=g4, e_g=e4)
    assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(list(g4.parameters()) + list(e4.parameters()), ema.params))
    # a blob written without an EMA
    checkpoint.save(prefix, 9, g=g, e_g=e_g, opt_g=opt_g)
    assert not os.path.exists('%s-genema-%05d' % (prefix, 9))
    with pytest.raises(KeyError):
        checkpoint.load(prefix, 9, g=g, e_g=e_g, opt_g=opt_g, ema=ema)
    with pytest.warns(UserWarning, match='EMA'):
        checkpoint.load(prefix, 9, g=g, e_g=e_g, opt_g=opt_g, ema=ema, strict=False)
    assert ema.step0 == 4 and all(torch.equal(s, p.detach().reshape(-1)) for s, p in zip(ema.shadows, ema.params))


# ------------------------------------------------------------------------------------------------------------------
# GPU: the HIP kernel
# ------------------------------------------------------------------------------------------------------------------
SENTINEL = 0x7FC0DEAD       # a NaN's bits, as int32


def _kernel_case(K):
    """-> (flat shadow buffer, shadows, params, mask of the shadows' elements, the parameters laid out like the buffer)"""
    ch = K.EMA_CHUNK
    gen = torch.Generator().manual_seed(5)
    sizes = [1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025, ch - 1, ch, ch + 1, 2 * ch + 3, 70001]
    sizes += [int(v) for v in torch.randint(1, 10, (300,), generator=gen)]
    # (numel, parameter offset from a 16-byte boundary in elements, shadow offset): the two views at storage offset 1 meet
    # aligned shadows (element-by-element path); then equally misaligned pairs (scalar head, 16-byte body, scalar tail)
    cases = [(n, 0, 0) for n in sizes] + [(6, 1, 0), (1030, 1, 0), (ch + 9, 1, 1), (2, 3, 3), (2 * ch, 2, 2), (5, 0, 2)]
    offs, o = [], 4
    for n, _, so in cases:
        offs.append(o + so)
        o = (o + so + n + 3) // 4 * 4 + 4              # (at least one 16-byte frame between two tensors)
    flat = torch.empty(o, dtype=torch.int32, device='cuda').fill_(SENTINEL).view(torch.float32)
    assert flat.data_ptr() % 16 == 0
    mask = torch.zeros(o, dtype=torch.bool, device='cuda')
    p_lay = torch.zeros(o, dtype=torch.float32, device='cuda')
    shadows, params, keep = [], [], []
    for (n, po, _), so in zip(cases, offs):
        scale = 10.0 ** float(torch.randint(-3, 4, (1,), generator=gen))
        buf = torch.empty(n + 4, device='cuda')
        assert buf.data_ptr() % 16 == 0
        p = buf[po:po + n]
        p.copy_((torch.randn(n, generator=gen) * scale).cuda())
        assert p.data_ptr() % 16 == 4 * po and p.storage_offset() == po
        keep.append(buf)
        params.append(p)
        shadows.append(flat[so:so + n])
        assert shadows[-1].data_ptr() % 16 == 4 * (so % 4)
        mask[so:so + n] = True
        p_lay[so:so + n] = p
    e_init = flat.clone()
    e_vals = (torch.randn(o, generator=gen) * 3.0).cuda()
    e_init[mask] = e_vals[mask]
    return flat, e_init, shadows, params, mask, p_lay, keep


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    return K_


@pytest.mark.gpu
def test_kernel_against_float64(K):
    flat, e_init, shadows, params, mask, p_lay, _ = _kernel_case(K)
    clones = [p.clone() for p in params]
    e64, p64 = e_init.double(), p_lay.double()
    scale = torch.maximum(e64.abs(), p64.abs())
    step0 = 7
    worst = 0.0
    for decay in (0.0, 0.5, 0.999, 1.0):
        for warmup in (True, False):
            for k in (1, 5, 100000):
                flat.copy_(e_init)
                step_dev = torch.tensor([step0 + k], dtype=torch.int32, device='cuda')
                K.ema_update(shadows, params, decay, warmup, step_dev, step0)
                w = weight(decay, warmup, k)
                want = e64 + float(w) * (p64 - e64)
                err = (flat.double() - want).abs()[mask]
                rel = float((err / scale[mask].clamp_min(1e-300)).max()) / 2.0 ** -24
                worst = max(worst, rel)
                print('decay %g warmup %d k %d: worst error %.3f units of 2^-24 max(|p|, |e|)' % (decay, warmup, k, rel))
                assert bool((err <= STEP_BOUND * scale[mask]).all()), (decay, warmup, k, rel)
                # the frames around every tensor keep their bits, the parameters and the counter are not written
                assert torch.equal(flat.view(torch.int32)[~mask], e_init.view(torch.int32)[~mask]), (decay, warmup, k)
                assert int(step_dev.item()) == step0 + k
                if w == 0:
                    assert decay == 1.0 and not warmup and torch.equal(flat.view(torch.int32), e_init.view(torch.int32))
                if w == 1:
                    assert decay == 0.0 and torch.equal(flat[mask], p_lay[mask])
    assert all(torch.equal(p, c) for p, c in zip(params, clones))
    # the host k when there is no device counter; a counter behind step0 counts as k = 0
    for step_dev, k_arg, k_eff in ((None, 5, 5), (torch.tensor([3], dtype=torch.int32, device='cuda'), 0, 0)):
        flat.copy_(e_init)
        K.ema_update(shadows, params, 0.999, True, step_dev, step0, k=k_arg)
        err = (flat.double() - (e64 + float(weight(0.999, True, k_eff)) * (p64 - e64))).abs()[mask]
        assert bool((err <= STEP_BOUND * scale[mask]).all()), k_eff
    with pytest.raises(ValueError):
        K.ema_update(shadows, params, 1.01, False, None, 0)
    with pytest.raises(ValueError):
        K.ema_update(shadows, params, -0.1, False, None, 0)
    with pytest.raises(RuntimeError):
        K.ema_update([s.cpu() for s in shadows[:2]], params[:2], 0.5, False, None, 0)
    print('worst of all cases: %.3f units' % worst)


@pytest.mark.gpu
def test_capture_reads_the_device_counter(K):
    from audiogan_amd import common, optim
    dev = 'cuda'
    ps, opt = _toy(dev)
    gen = torch.Generator().manual_seed(9)
    for p in ps[:-1]:
        p.grad = torch.randn(p.shape, generator=gen).to(dev)          # constant gradients
    ema = optim.EMA(opt, decay=0.999, warmup=True)

    def step():
        opt.step()
        ema.update()

    step()
    step()
    torch.cuda.synchronize()
    snap = ([p.detach().clone() for p in ps], opt.state_dict(), ema.state_dict())
    K.reserve_table_arena()
    mark = K.capture_mark()
    gr = torch.cuda.CUDAGraph()
    common.new_capture()
    try:
        with torch.cuda.graph(gr, capture_error_mode='thread_local'):
            step()
    except Exception:
        K.drop_captured_tables(mark)
        raise
    torch.cuda.synchronize()
    # (capturing executes nothing)
    assert all(torch.equal(p.detach(), q) for p, q in zip(ps, snap[0]))
    assert all(torch.equal(s, t) for s, t in zip(ema.shadows, snap[2]['shadows']))
    hist = []
    for _ in range(20):
        gr.replay()
        hist.append(([p.detach().clone() for p in ps], [s.clone() for s in ema.shadows]))
    torch.cuda.synchronize()
    # 5 replays == 5 eager steps from the same state
    with torch.no_grad():
        for p, q in zip(ps, snap[0]):
            p.copy_(q)
    opt.load_state_dict(snap[1])
    ema.load_state_dict(snap[2])
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    for i, p in enumerate(ps):
        assert torch.equal(p.detach(), hist[4][0][i]), i
        assert torch.equal(ema.shadows[i], hist[4][1][i]), i
    # float64 over the recorded parameters: k runs 3, 4, ... (two eager steps came first); a decay frozen at its
    # capture-time value (k = 3 on every replay) is something else
    ref = [s.double() for s in snap[2]['shadows']]
    froz = [s.double() for s in snap[2]['shadows']]
    mx = [r.abs() for r in ref]
    for j, (pj, sj) in enumerate(hist):
        for i in range(len(ps)):
            mx[i] = torch.maximum(mx[i], pj[i].double().reshape(-1).abs())
            ref[i] = lerp64(ref[i], pj[i].reshape(-1), weight(0.999, True, 3 + j))
            froz[i] = lerp64(froz[i], pj[i].reshape(-1), weight(0.999, True, 3))
            _within(sj[i], ref[i], (j + 1) * STEP_BOUND * mx[i], 'replay %d tensor %d' % (j, i))
        if j == 4:
            for i in range(len(ps) - 1):
                assert not torch.allclose(sj[i].double(), froz[i], rtol=1e-3, atol=0), i
    assert torch.equal(hist[-1][1][-1], snap[0][-1].reshape(-1))           # (the parameter without a gradient)
    assert int(opt._state['step'].item()) == 7


WORDS8 = (np.random.RandomState(0).randint(97, 123, size=(8, 5)), np.array([5, 3, 4, 2, 5, 1, 2, 3]))
GCFG_GPU = dict(frame_size=40, embed_size=8, noise_size=8, state_size=128, num_layers=1, struct=[[17, 8, 16, 8], [9, 4, 16, 8]])


def _gpu_loop(A, tmp_path, graphed, with_ema, passes, **kw):
    from audiogan_amd import optim
    from tests.test_gpu_front_frames import _loop_setup
    dev = torch.device('cuda')
    mk, mods = _loop_setup(A, dev, tmp_path, 8)
    torch.cuda.manual_seed(17)
    ema = optim.EMA(mk(checkpoint_every=0).opt_g, decay=0.99, warmup=True) if with_ema else None
    args = dict(fixed_critic_iter=2, gencatchup=1, stop='never', checkpoint_every=0, check=False, graphed=graphed, host=False)
    if with_ema:
        args.update(ema=ema, sample_every=2, sample_words=WORDS8, sample_seed=3)
    args.update(kw)
    lp = mk(**args)
    for _ in range(passes):
        lp.outer()
    torch.cuda.synchronize()
    return lp, mods, ema


@pytest.mark.gpu
def test_loop_eager_against_captured(K, tmp_path):
    import audiogan_amd as A
    K.lstm_persist_status(reset=True)
    waves = [[], []]
    got = []
    for graphed in (False, True):
        lp, mods, ema = _gpu_loop(A, tmp_path, graphed, True, 4 if graphed else 6,
                                  on_sample=lambda n, w, ln, sl, graphed=graphed: waves[int(graphed)].append((n, w.clone())))
        assert lp.dis_iter == 12 and lp.gen_iter == 6 and (lp._graphs is not None) == graphed
        got.append(([p.detach().clone() for m in mods for p in m.parameters()], [s.clone() for s in ema.shadows],
                    [p.detach().clone() for p in ema.params]))
    for a, b in zip(got[0][0] + got[0][1], got[1][0] + got[1][1]):
        assert torch.equal(a, b)
    assert [n for n, _ in waves[0]] == [2, 4, 6] == [n for n, _ in waves[1]]
    assert all(torch.equal(a, b) for (_, a), (_, b) in zip(waves[0], waves[1]))
    assert sum(int(not torch.equal(s, p.reshape(-1))) for s, p in zip(got[1][1], got[1][2])) > 0.5 * len(got[1][1])
    lp, mods, _ = _gpu_loop(A, tmp_path, True, False, 4)
    for a, p in zip(got[1][0], [p for m in mods for p in m.parameters()]):
        assert torch.equal(a, p.detach())
    assert K.lstm_persist_status() == 0


@pytest.mark.gpu
def test_sampling_leaves_the_weight_caches_right(K, tmp_path):
    import audiogan_amd as A
    lp, mods, ema = _gpu_loop(A, tmp_path, False, True, 2, sample_every=0)
    g = mods[0]
    gen = torch.Generator().manual_seed(11)
    T = 6
    z, c = torch.randn(8, T, 8, generator=gen).cuda(), torch.randn(8, 8, generator=gen).cuda()
    u = torch.rand(T, 8, generator=gen).cuda()
    first = g(z=z, c=c, stop='never')[0].detach().clone()
    with ema.applied():
        wave, s, _, length = g.generate(c, z=z, u=u)
        sd = ema.module_state_dict(g)
    g2 = A.Generator(**GCFG_GPU).cuda()
    g2.load_state_dict(sd, strict=True)
    wave2, s2, _, length2 = g2.generate(c, z=z, u=u)
    assert torch.equal(wave, wave2) and torch.equal(s, s2) and torch.equal(length, length2)
    raw = g.generate(c, z=z, u=u)[0]
    assert raw.shape != wave.shape or not torch.equal(raw, wave)          # (the average is not the last iterate)
    again = g(z=z, c=c, stop='never')[0].detach()
    assert torch.equal(first, again)
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0
