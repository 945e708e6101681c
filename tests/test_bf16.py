"""BASELINE configs[2] (bf16): audiogan_amd's AG_PREC_BF16 mode - every contraction rounds both operands to bfloat16
(RNE) and accumulates in fp32 - against (a) torch ops on rounded operands, kernel by kernel, and (b) the CPU oracle's
``bf16_mode`` (oracle/audiogan_oracle.py), module by module and for a whole G+D step.

DECLARED TOLERANCE:
  * one contraction vs the same contraction on rounded operands in fp32: 1e-4 of the output scale (the products are
    exact in fp32; only the order of the fp32 additions differs);
  * networks / train step vs the bf16-rounded oracle: every activation / logit / waveform tensor within 1e-2 of its
    largest magnitude elementwise and 3e-3 in relative L2 norm (an intermediate value that differs in the last fp32
    bits can round to the other bf16 neighbour, a 2^-8 relative change of that one element); parameter gradients
    (sums over batch and time in which such flips do not cancel) 2e-2 in relative L2 norm and 5e-2 of the largest
    magnitude elementwise (the worst of up to a million elements); the weight-norm gain gradients, cancelling projections
    two orders of magnitude smaller, 5e-2 in both;
  * vs the fp32 oracle: 3e-2 in relative L2 norm (what bf16 operands cost; informative).
  * bf16 STORAGE (round 4): where the critic's sequence path is kept as bfloat16 in HBM (Discriminator.stores_bf16) the
    oracle runs ``bf16_mode(store=True)``, which rounds those tensors - value and gradient - where they are written; the
    same tolerances apply.  ag_gemm_h alone: fp32 output within 1e-4 of the output scale of a float64 product of the same
    bf16 operands, a bf16 output within one bf16 ulp (2^-8 relative) of that product."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import audiogan_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available()
    import audiogan_amd.kernels as K
    return K


@pytest.fixture()
def bf16(K):
    old = K.set_precision('bf16')
    yield
    K.set_precision(old)


def rnd(t):
    return t.bfloat16().float()


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


# activations / logits on the bf16-STORAGE path (round 4): every stored tensor is one more rounding point at which two
# implementations of the same contract can land on different bf16 neighbours, so the relative-L2 bound of such tensors is
# declared at 5e-3 (fp32 storage: 3e-3, about half as many rounding points); elementwise bound unchanged
L2_STORE = 5e-3


def close_bf16(got, ref, msg='', elem=1e-2, l2=3e-3):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    scale = float(ref.abs().max())
    assert float((got - ref).abs().max()) <= elem * max(scale, 1e-6), (msg, float((got - ref).abs().max()), scale)
    if scale > 0:
        assert rel_l2(got, ref) <= l2, (msg, rel_l2(got, ref))


@pytest.mark.parametrize('shape', [(8192, 1024, 1024), (2048, 512, 1480), (130, 70, 36), (64, 4096, 1480),
                                   (4096, 1480, 8192), (40, 36, 8)])
@pytest.mark.parametrize('ta,tb', [(False, True), (False, False), (True, False), (True, True)])
def test_gemm_bf16(K, bf16, shape, ta, tb):
    M, N, Kd = shape
    gen = torch.Generator().manual_seed(3)
    A = torch.randn((Kd, M) if ta else (M, Kd), generator=gen)
    B = torch.randn((N, Kd) if tb else (Kd, N), generator=gen)
    bias, res = torch.randn(N, generator=gen), torch.randn(M, N, generator=gen)
    ref = (rnd(A).t() if ta else rnd(A)).double() @ (rnd(B).t() if tb else rnd(B)).double()
    ref = F.leaky_relu(ref + bias.double() + res.double(), 0.01)
    out = torch.empty(M, N).cuda()
    K.gemm(A.cuda(), B.cuda(), out, ta=ta, tb=tb, bias=bias.cuda(), res=res.cuda(), act=K.ACT_LEAKY)
    err = float((out.cpu().double() - ref).abs().max())
    assert err <= 1e-4 * float(ref.abs().max()), (shape, ta, tb, err)
    # the fp32 result of the UNROUNDED operands is further away: the mode really rounds
    full = F.leaky_relu((A.t() if ta else A).double() @ (B.t() if tb else B).double() + bias.double() + res.double(), 0.01)
    if Kd >= 36:
        assert float((out.cpu().double() - full).abs().max()) > 10 * err


def test_gemm_bf16_splitk_weight_gradient(K, bf16):
    """few output tiles, long reduction (a weight gradient): split-K slabs + fixed-order sum, also in bf16 mode"""
    gen = torch.Generator().manual_seed(4)
    dy, x = torch.randn(16384, 512, generator=gen), torch.randn(16384, 256, generator=gen)
    out = torch.zeros(512, 256).cuda()
    K.gemm(dy.cuda(), x.cuda(), out, ta=True, beta=1.0)
    ref = rnd(dy).double().t() @ rnd(x).double()
    assert float((out.cpu().double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    out2 = torch.zeros(512, 256).cuda()
    K.gemm(dy.cuda(), x.cuda(), out2, ta=True, beta=1.0)
    assert torch.equal(out, out2)


LAYERS = [('conv', 1, 128, 17, 8, 8, 2048), ('convT', 128, 16, 16, 8, 4, 256), ('conv', 49, 64, 9, 4, 4, 2048),
          ('convT', 64, 32, 8, 4, 2, 512), ('conv', 113, 1, 3, 1, 1, 2048), ('conv', 64, 128, 7, 2, 3, 1024),
          ('conv', 256, 512, 7, 2, 3, 256), ('conv', 17, 64, 9, 4, 4, 2048), ('conv', 256, 256, 7, 2, 3, 250),
          ('convT', 32, 32, 8, 4, 2, 2048), ('conv', 81, 32, 9, 4, 4, 4096), ('conv', 24, 40, 5, 3, 2, 301),
          ('convT', 40, 24, 6, 3, 1, 99)]


@pytest.mark.parametrize('layer', LAYERS)
def test_conv_layers_bf16(K, bf16, layer):
    """forward, backward-data and backward-weight of C2 layer shapes vs torch convs on rounded operands"""
    from audiogan_amd import ops
    kind, cin, cout, k, s, p, lin = layer
    B = 3
    gen = torch.Generator().manual_seed(6)
    spec = ops.ConvSpec(kind, cin, cout, k, s, p)
    w = torch.randn((cout, cin, k) if kind == 'conv' else (cin, cout, k), generator=gen) / (cin * k) ** 0.5
    x = torch.randn(B, cin, lin, generator=gen)
    lout = spec.out_len(lin)
    dy = torch.randn(B, cout, lout, generator=gen)
    xr, wr, dyr = rnd(x).double().requires_grad_(True), rnd(w).double().requires_grad_(True), rnd(dy).double()
    yr = F.conv1d(xr, wr, None, s, p) if kind == 'conv' else F.conv_transpose1d(xr, wr, None, s, p)
    yr.backward(dyr)
    d0, d1, _ = w.shape
    prep = ops.Prepared(w=w.cuda(), wpa=torch.zeros(K.wpa_numel(d0, d1, k)).cuda(),
                        wpb=torch.zeros(K.wpb_numel(d0, d1, k, s)).cuda(), pad=p)
    K.prep_conv_weight(prep.w, prep.wpa, prep.wpb, s, p)
    y = torch.empty(B, cout, lout).cuda()
    ops.conv_fwd(spec, prep, x.cuda(), y)
    dx = torch.empty(B, cin, lin).cuda()
    ops.conv_bwd_data(spec, prep, dy.cuda(), dx)
    dw = torch.zeros_like(w).cuda()
    ops.conv_wgrad(spec, x.cuda(), dy.cuda(), dw, None)
    for got, ref, n in ((y, yr, 'y'), (dx, xr.grad, 'dx'), (dw, wr.grad, 'dw')):
        err = float((got.cpu().double() - ref.detach()).abs().max())
        assert err <= 1e-4 * float(ref.abs().max()), (layer, n, err)


def _small_models(A):
    gcfg = dict(frame_size=64, embed_size=16, noise_size=16, state_size=128, num_layers=1,
                struct=[[17, 8, 32, 8], [9, 4, 32, 16], [9, 4, 16, 16]])
    dcfg = dict(state_size=128, embed_size=16, num_layers=1, cnn_struct=[[7, 2, 8], [7, 2, 16], [7, 2, 32], [7, 2, 64]])
    torch.manual_seed(31)
    go, do = O.Generator(**gcfg), O.Discriminator(**dcfg)
    g, d = A.Generator(**gcfg), A.Discriminator(**dcfg)
    g.load_state_dict(go.state_dict()); d.load_state_dict(do.state_dict())
    return go, do, g.cuda(), d.cuda()


def test_networks_bf16_vs_rounded_oracle(K, bf16):
    """G and D (ragged lengths; persistent biLSTM kernels, split GEMMs, every conv class) forward + backward in bf16
    mode vs the oracle's bf16_mode, and - informative bound - vs the fp32 oracle"""
    import audiogan_amd as A
    go, do, g, d = _small_models(A)
    B, T, fs = 16, 16, 64
    gen = torch.Generator().manual_seed(32)
    z, c = torch.randn(B, T, 16, generator=gen), torch.randn(B, 16, generator=gen)
    lens = torch.randint(300, T * fs + 1, (B,), generator=gen)
    lens[0] = T * fs
    wl = torch.randn(B, T * fs // 16, generator=gen)
    stop = torch.zeros(B, T, dtype=torch.long)
    x32 = go(z=z, c=c, stop=stop)[0]
    l32 = do(x32, lens, c)[0]
    with O.bf16_mode(store=d.stores_bf16(B, 'cuda')):
        xo = go(z=z, c=c, stop=stop)[0]
        xo.retain_grad()
        lo, actso, _, _ = do(xo, lens, c)
        (lo * wl).sum().backward()
    x = g(z=z.cuda(), c=c.cuda(), stop='never')[0]
    x.retain_grad()
    l, acts, _, _ = d(x, lens.cuda(), c.cuda())
    (l * wl.cuda()).sum().backward()
    close_bf16(x, xo, 'waveform')
    close_bf16(l, lo, 'logits')
    for i, (a, b) in enumerate(zip(acts, actso)):
        close_bf16(a, b, 'act%d' % i)
    # the critic's input gradient first: it is what the generator's gradients are made of (a mismatch further down with
    # this one green points at the generator's backward, red at the critic's).
    # (1) the critic ALONE: the oracle's waveform fed to the HIP critic - same point, so the declared activation-class bound
    #     holds (measured 3.4e-3 of the largest entry, 1.3e-3 relative L2: tools/diag_bf16_xgrad.py)
    from audiogan_amd.common import frozen
    xs = xo.detach().clone().cuda().requires_grad_(True)
    with frozen(d):          # (an input-gradient pass: the blocks' backward must not add to the weights' .grad a second time)
        ls = d(xs, lens.cuda(), c.cuda())[0]
        gs, = torch.autograd.grad((ls * wl.cuda()).sum(), xs)
    close_bf16(gs, xo.grad, 'd(loss)/d(waveform), same waveform', elem=1e-2, l2=3e-3)
    # (2) end to end each critic reads ITS OWN generator's waveform (2.5e-4 apart in relative L2), i.e. the two gradients are
    #     taken at different points: a LeakyReLU unit whose pre-activation is within that distance of zero takes the other
    #     branch on one side (1-2 units of 262144 here) and the input positions in its receptive field move by up to 7 % of
    #     the tensor's maximum.  The conv activations of both sides say which units flipped: outside their receptive fields
    #     the same-point bound must hold, inside them 0.2 (the bound is now derived, not fitted).
    under = torch.zeros(x.shape, dtype=torch.bool)
    nflip = 0
    for i, (a, b) in enumerate(zip(acts, actso)):
        flip = (a.detach().cpu() > 0) != (b.detach() > 0)
        nflip += int(flip.sum())
        stride, R = 2 ** (i + 1), 3 * (2 ** (i + 1) - 1)            # k7 s2 p3 layers: field of unit u of layer i
        for bb, u in flip.any(1).nonzero().tolist():
            under[bb, max(0, u * stride - R):min(x.size(1), u * stride + R + 1)] = True
    assert nflip <= 1e-4 * sum(a.numel() for a in acts) and float(under.float().mean()) <= 0.05, (nflip, float(under.float().mean()))
    ge, gscale = (x.grad.cpu() - xo.grad).abs(), float(xo.grad.abs().max())
    assert float(ge[~under].max()) <= 1e-2 * gscale, ('d(loss)/d(waveform) outside flipped units', float(ge[~under].max()) / gscale)
    close_bf16(x.grad, xo.grad, 'd(loss)/d(waveform)', elem=0.2, l2=2e-2)
    for mod, ref in ((d, do), (g, go)):
        rp = dict(ref.named_parameters())
        for k, q in mod.named_parameters():
            if k.split('.')[-1].startswith('bias') and k.endswith('_v'):
                continue
            r = rp[k].grad if rp[k].grad is not None else torch.zeros_like(rp[k])
            close_bf16(q.grad if q.grad is not None else torch.zeros_like(q), r, k, elem=5e-2,
                       l2=5e-2 if k.endswith('_g') else 2e-2)
    assert rel_l2(x, x32) <= 3e-2 and rel_l2(l, l32) <= 3e-2
    assert rel_l2(x, x32) > 1e-5          # (and the mode is really on)


def test_train_step_bf16_vs_rounded_oracle(K, bf16):
    import audiogan_amd as A
    from audiogan_amd import optim, train
    go, do, g, d = _small_models(A)
    B, T, fs = 8, 16, 64
    gen = torch.Generator().manual_seed(33)
    real = torch.rand(B, T * fs, generator=gen) * 2 - 1
    rl = torch.full((B,), T * fs, dtype=torch.long)
    c, z = torch.randn(B, 16, generator=gen), torch.randn(B, T, 16, generator=gen)
    nr, nf = torch.randn(B, T * fs, generator=gen) * 0.01, torch.randn(B, T * fs, generator=gen) * 0.01
    stop = torch.zeros(B, T, dtype=torch.long)
    opt_do, opt_go = O.make_optimizer(list(do.parameters()), 'adam', 1e-4), O.make_optimizer(list(go.parameters()), 'adam', 1e-4)
    opt_d, opt_g = optim.make_optimizer(list(d.parameters()), 'adam', 1e-4), optim.make_optimizer(list(g.parameters()), 'adam', 1e-4)
    cu = lambda t: t.cuda()  # noqa: E731
    assert d.stores_bf16(2 * B, 'cuda') == d.stores_bf16(B, 'cuda')
    with O.bf16_mode(store=d.stores_bf16(B, 'cuda')):
        lo, cdo, cgo = O.d_step(go, do, opt_do, real, rl, c, z, nr, nf, 1.0, stop=stop)
        lo2, fo, _ = O.g_step(go, do, opt_go, c, z, nf, 0.1, stop=stop)
    l, cd, cg = train.d_step(g, d, opt_d, cu(real), cu(rl), cu(c), cu(z), cu(nr), cu(nf), 1.0, check=True)
    l2, f, _ = train.g_step(g, d, opt_g, cu(c), cu(z), cu(nf), 0.1, check=True)
    close_bf16(cd, cdo, 'D(real)'); close_bf16(cg, cgo, 'D(fake)'); close_bf16(f, fo, 'fake')
    np.testing.assert_allclose([float(l), float(l2)], [float(lo), float(lo2)], rtol=2e-3)


@pytest.mark.parametrize('B', [40, 70])
def test_bf16_mfma_persistent_recurrent_kernels(K, bf16, B):
    """shapes that take the bf16-MFMA forms of the persistent launches (H = 512 per direction: v_mfma_f32_32x32x16_bf16
    forward with the W_hh slice in LDS as bf16, v_mfma_f32_16x16x32_bf16 backward; S = 1024 / frame 256 generator
    front) vs the bf16-rounded oracle: critic logits, generated frames and all gradients"""
    import audiogan_amd as A
    dcfg = dict(state_size=1024, embed_size=8, num_layers=1, cnn_struct=[[7, 2, 8], [7, 2, 16]])
    gcfg = dict(frame_size=256, embed_size=8, noise_size=8, state_size=1024, num_layers=1, struct=[[9, 4, 8, 4]])
    torch.manual_seed(41)
    do, go = O.Discriminator(**dcfg), O.Generator(**gcfg)
    d, g = A.Discriminator(**dcfg), A.Generator(**gcfg)
    d.load_state_dict(do.state_dict()); g.load_state_dict(go.state_dict())
    d.cuda(); g.cuda()
    gen = torch.Generator().manual_seed(42)
    L = 64
    x, c = torch.randn(B, L, generator=gen), torch.randn(B, 8, generator=gen)
    lens = torch.randint(20, L + 1, (B,), generator=gen)
    lens[0] = L
    wl = torch.randn(B, L // 4, generator=gen)
    with O.bf16_mode(store=d.stores_bf16(B, 'cuda')):
        lo = do(x, lens, c)[0]
        (lo * wl).sum().backward()
    l = d(x.cuda(), lens.cuda(), c.cuda())[0]
    (l * wl.cuda()).sum().backward()
    assert K.lstm_persist_status() == 0
    close_bf16(l, lo, 'logits')
    rp = dict(do.named_parameters())
    # (parameter gradients off the bf16-storage path: about twice the rounding points of fp32 storage - the worst single
    # element of up to a million is declared at 8e-2 of the tensor's largest entry there, 5e-2 on fp32 storage; L2 unchanged)
    elem_p = 8e-2 if d.stores_bf16(B, 'cuda') else 5e-2
    for k, q in d.named_parameters():
        if k.split('.')[-1].startswith('bias') and k.endswith('_v'):
            continue
        close_bf16(q.grad, rp[k].grad, k, elem=elem_p, l2=5e-2 if k.endswith('_g') else 2e-2)
    if B <= 64:
        T = 3
        z = torch.randn(B, T, 8, generator=gen)
        wx = torch.randn(B, T * 256, generator=gen)
        with O.bf16_mode():
            xo = go(z=z, c=c, stop=torch.zeros(B, T, dtype=torch.long))[0]
            (xo * wx).sum().backward()
        xg = g(z=z.cuda(), c=c.cuda(), stop='never')[0]
        (xg * wx.cuda()).sum().backward()
        assert K.lstm_persist_status() == 0
        close_bf16(xg, xo, 'waveform')
        rp = dict(go.named_parameters())
        for k, q in g.named_parameters():
            if (k.split('.')[-1].startswith('bias') and k.endswith('_v')) or rp[k].grad is None:
                continue
            close_bf16(q.grad, rp[k].grad, k, elem=5e-2, l2=5e-2 if k.endswith('_g') else 2e-2)


@pytest.mark.parametrize('shape', [(8192, 1024, 1024), (2048, 2048, 1480), (4096, 1480, 8192)])
@pytest.mark.parametrize('ta,tb', [(False, True), (False, False), (True, False)])
def test_gemm_f32x3_experiment(K, shape, ta, tb):
    """AG_PREC_F32X3 (an experiment, bench.py --dtype f32x3): bf16 hi + lo split of both operands, three bf16 MFMAs per
    product.  Error bound per product 2^-16 relative (the dropped lo*lo term and the rounding of lo); measured against
    float64: within 2e-5 of the output scale, ~100x closer than the plain bf16 mode"""
    M, N, Kd = shape
    gen = torch.Generator().manual_seed(5)
    A = torch.randn((Kd, M) if ta else (M, Kd), generator=gen)
    B = torch.randn((N, Kd) if tb else (Kd, N), generator=gen)
    ref = (A.t() if ta else A).double() @ (B.t() if tb else B).double()
    out = torch.empty(M, N).cuda()
    old = K.set_precision('f32x3')
    try:
        K.gemm(A.cuda(), B.cuda(), out, ta=ta, tb=tb)
    finally:
        K.set_precision(old)
    err = float((out.cpu().double() - ref).abs().max()) / float(ref.abs().max())
    assert err <= 2e-5, (shape, ta, tb, err)
    out32 = torch.empty(M, N).cuda()
    K.gemm(A.cuda(), B.cuda(), out32, ta=ta, tb=tb)
    assert not torch.equal(out, out32), 'the mode did not take the split-bf16 kernel'


# ---------------------------------------------------------------------------------------------------------------------
# bf16 STORAGE (round 4): ag_gemm_h on operands stored as bfloat16, and the storage variants of the kernels around it
# ---------------------------------------------------------------------------------------------------------------------
def _b16(*shape, gen, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(torch.bfloat16)


@pytest.mark.parametrize('shape', [(8192, 1024, 1024), (2048, 512, 2048), (384, 200, 128), (128, 128, 64), (16384, 2048, 512),
                                   (8200, 1000, 128)])      # (ragged tiles in both directions on a full-chip grid)
@pytest.mark.parametrize('ta,tb', [(False, True), (False, False), (True, False), (True, True)])
def test_gemm_h_all_operand_layouts(K, shape, ta, tb):
    """k-contiguous operands through ds_read_b128, k-strided ones through the transposed LDS read, LDS-DMA staging with both
    swizzles: every (ta, tb), fp32 and bf16 outputs, against a float64 product of the same bf16 values"""
    M, N, Kd = shape
    gen = torch.Generator().manual_seed(M + 3 * N + 7 * Kd + 2 * ta + tb)
    a = _b16(*((Kd, M) if ta else (M, Kd)), gen=gen)
    b = _b16(*((N, Kd) if tb else (Kd, N)), gen=gen)
    ref = (a.double().t() if ta else a.double()) @ (b.double().t() if tb else b.double())
    A, B = a.cuda(), b.cuda()
    assert K.gemm_h_ok(A, B, ta, tb)
    c32 = torch.full((M, N), float('nan')).cuda()
    c16 = torch.full((M, N), float('nan'), dtype=torch.bfloat16).cuda()
    K.gemm_h(A, B, C=c32, C16=c16, ta=ta, tb=tb)
    scale = float(ref.abs().max())
    assert float((c32.cpu().double() - ref).abs().max()) <= 1e-4 * scale
    got16, want16 = c16.float().cpu().double(), ref.float().bfloat16().double()
    assert float((got16 - want16).abs().max()) <= 2.0 ** -7 * scale       # one bf16 ulp at the top of the range
    assert float(((got16 - want16).abs() > 0).double().mean()) < 0.02       # (ties / last-bit sums only)


def test_gemm_h_epilogues_at_full_size(K):
    """the epilogue forms of the critic's heads at the critic's size (a full-chip grid of tiles through the LDS-transposed
    epilogue): bias + bf16 residual + LeakyReLU to a bf16 output, fp32 residual into a pitched fp32 view, the gate forms, beta = 1"""
    gen = torch.Generator().manual_seed(78)
    M, N, Kd = 8192, 1024, 256
    a, w = _b16(M, Kd, gen=gen).cuda(), _b16(N, Kd, gen=gen, scale=0.05).cuda()
    bias = torch.randn(N, generator=gen).cuda()
    res16, res32 = _b16(M, N, gen=gen).cuda(), torch.randn(M, N, generator=gen).cuda()
    lin = a.double() @ w.double().t() + bias.double()
    y16 = torch.empty(M, N, dtype=torch.bfloat16).cuda()
    K.gemm_h(a, w, C16=y16, tb=True, bias=bias, res=res16, act=K.ACT_LEAKY)
    ref = F.leaky_relu(lin + res16.double(), 0.01)
    assert float((y16.double() - ref.float().bfloat16().double()).abs().max()) <= 2.0 ** -7 * float(ref.abs().max())
    wide = torch.zeros(M, N + 24).cuda()
    K.gemm_h(a, w, C=wide[:, 8:8 + N], tb=True, bias=bias, res=res32)
    assert float((wide[:, 8:8 + N].double() - (lin + res32.double())).abs().max()) <= 1e-4 * float(lin.abs().max())
    assert not wide[:, :8].any() and not wide[:, 8 + N:].any()
    K.gemm_h(a, w, C=wide[:, 8:8 + N], tb=True, beta=1.0)                     # accumulate on top
    assert float((wide[:, 8:8 + N].double() - (2 * lin - bias.double() + res32.double())).abs().max()) <= 2e-4 * float(lin.abs().max())
    da, sv = _b16(M, N, gen=gen).cuda(), _b16(M, N, gen=gen).cuda()
    w2 = _b16(N, N, gen=gen, scale=0.05).cuda()
    dp = torch.empty(M, N, dtype=torch.bfloat16).cuda()
    K.gemm_h(da, w2, C16=dp, res=da, gate=sv)
    ref = (da.double() @ w2.double() + da.double()) * torch.where(sv.double() > 0, 1.0, 0.01)
    assert float((dp.double() - ref.float().bfloat16().double()).abs().max()) <= 2.0 ** -7 * float(ref.abs().max())
    K.gemm_h(da, w2, C16=dp, res=sv, act=K.ACT_LEAKY_GATE)
    ref = (da.double() @ w2.double()) * torch.where(sv.double() > 0, 1.0, 0.01)
    assert float((dp.double() - ref.float().bfloat16().double()).abs().max()) <= 2.0 ** -7 * float(ref.abs().max())


def test_gemm_h_epilogues_views_and_split_k(K):
    """bias, fp32 / bf16 residuals, LeakyReLU, the gate forms, pitched operand views and outputs, and the split-K weight
    gradient (beta = 1, deferred second stage) - the forms the critic's heads and biLSTM use"""
    gen = torch.Generator().manual_seed(77)
    M, N, Kd = 1024, 512, 1024
    a, w = _b16(M, Kd, gen=gen).cuda(), _b16(N, Kd, gen=gen, scale=0.05).cuda()
    bias = torch.randn(N, generator=gen).cuda()
    res16 = _b16(M, N, gen=gen).cuda()
    res32 = torch.randn(M, N, generator=gen).cuda()
    lin = a.double() @ w.double().t() + bias.double()
    # forward of a residual layer: LeakyReLU(a W^T + b + res), bf16 out
    y16 = torch.empty(M, N, dtype=torch.bfloat16).cuda()
    K.gemm_h(a, w, C16=y16, tb=True, bias=bias, res=res16, act=K.ACT_LEAKY)
    ref = F.leaky_relu(lin + res16.double(), 0.01)
    assert float((y16.double() - ref.float().bfloat16().double()).abs().max()) <= 2.0 ** -7 * float(ref.abs().max())
    # fp32 residual + fp32 out, into a pitched view
    wide = torch.zeros(M, N + 24).cuda()
    K.gemm_h(a, w, C=wide[:, 8:8 + N], tb=True, bias=bias, res=res32)
    assert float((wide[:, 8:8 + N].double() - (lin + res32.double())).abs().max()) <= 1e-4 * float(lin.abs().max())
    assert not wide[:, :8].any() and not wide[:, 8 + N:].any()
    # data gradient of a residual layer: (da W + da) gated by the saved activation below; W read k-strided
    da, sv = _b16(M, N, gen=gen).cuda(), _b16(M, N, gen=gen).cuda()
    w2 = _b16(N, N, gen=gen, scale=0.05).cuda()
    dp = torch.empty(M, N, dtype=torch.bfloat16).cuda()
    K.gemm_h(da, w2, C16=dp, res=da, gate=sv)
    ref = (da.double() @ w2.double() + da.double()) * torch.where(sv.double() > 0, 1.0, 0.01)
    assert float((dp.double() - ref.float().bfloat16().double()).abs().max()) <= 2.0 ** -7 * float(ref.abs().max())
    # ACT_LEAKY_GATE with the saved activation as `res`
    K.gemm_h(da, w2, C16=dp, res=sv, act=K.ACT_LEAKY_GATE)
    ref = (da.double() @ w2.double()) * torch.where(sv.double() > 0, 1.0, 0.01)
    assert float((dp.double() - ref.float().bfloat16().double()).abs().max()) <= 2.0 ** -7 * float(ref.abs().max())
    # weight gradient dW += dY^T X over 16384 rows: split-K, both operands k-strided column blocks of wider tensors
    R = 16384
    dy, x = _b16(R, 2 * N, gen=gen, scale=0.1).cuda(), _b16(R, 640, gen=gen).cuda()
    dyv, xv = dy[:, N:], x[:, 64:576]
    base = torch.randn(N, 612, generator=gen).cuda()
    ref = base[:, :512].double() + dyv.double().t() @ xv.double()
    assert K.lib.ag_gemm_h_ws_numel(N, 512, R, 0, 0) > 0
    plain, deferred = base.clone(), base.clone()
    K.gemm_h(dyv, xv, C=plain[:, :512], ta=True, beta=1.0)
    with K.deferred_reduces():
        K.gemm_h(dyv, xv, C=deferred[:, :512], ta=True, beta=1.0, defer=True)
        torch.cuda.synchronize()
        assert torch.equal(deferred, base), 'the deferred second stage ran before the flush'
    torch.cuda.synchronize()
    assert torch.equal(plain, deferred)
    assert torch.equal(plain[:, 512:], base[:, 512:])
    assert float((plain[:, :512].double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())


def test_bf16_storage_variants_of_the_small_kernels(K, bf16):
    """transposes, rowdot forward / backward and column sums with bfloat16 on the storage side vs the fp32 forms"""
    gen = torch.Generator().manual_seed(78)
    B, Cc, T = 6, 40, 33
    a = torch.randn(B, Cc, T, generator=gen).cuda()
    t16 = K.bct_to_tbc(a, out_dtype=torch.bfloat16)
    assert t16.dtype == torch.bfloat16 and torch.equal(t16, a.permute(2, 0, 1).contiguous().to(torch.bfloat16))
    back = K.tbc_to_bct(t16, out_dtype=torch.float32)
    assert torch.equal(back, t16.float().permute(1, 2, 0).contiguous())
    M, Kd = 300, 512
    x16 = _b16(M, Kd, gen=gen).cuda()
    w, b1 = (torch.randn(1, Kd, generator=gen) * 0.05).cuda(), torch.randn(1, generator=gen).cuda()
    y = torch.empty(M, 1).cuda()
    K.rowdot_fwd(x16, w, b1, y)
    ref = x16.double() @ rnd(w).double().t() + b1.double()
    assert float((y.double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    dy = torch.randn(M, 1, generator=gen).cuda()
    flat = torch.zeros(Kd + 1).cuda()
    dw, db = flat[:Kd].view(1, Kd), flat[Kd:]
    dx16 = torch.empty(M, Kd, dtype=torch.bfloat16).cuda()
    K.rowdot_bwd(dy, x16, w, dx=dx16, dw=dw, db=db, gate=True)
    g = rnd(dy).double()
    refdx = (g * rnd(w).double()) * torch.where(x16.double() > 0, 1.0, 0.01)
    assert float((dx16.double() - refdx.float().bfloat16().double()).abs().max()) <= 2.0 ** -7 * float(refdx.abs().max())
    refdw = (g * x16.double()).sum(0)
    assert float((dw.double().view(-1) - refdw).abs().max()) <= 1e-4 * float(refdw.abs().max())
    assert abs(float(db) - float(dy.double().sum())) <= 1e-4 * float(dy.abs().sum())
    out = torch.zeros(Kd).cuda()
    K.col_sum(x16, out)
    assert float((out.double() - x16.double().sum(0)).abs().max()) <= 1e-4 * float(x16.double().sum(0).abs().max())


def test_critic_sequence_path_bf16_storage_vs_fp32_storage(K, bf16):
    """the critic's classify() - time-major transpose, biLSTM (persistent launches writing y / reading dy as bf16, dgates'
    bf16 copy), heads - on bf16 storage against the same precision mode on fp32 storage (AG_BF16_STORE off): logits and
    every gradient inside the declared bf16 tolerance, and really on the bf16 kernels"""
    import audiogan_amd as A
    torch.manual_seed(41)
    d = A.Discriminator(state_size=256, embed_size=16, num_layers=1, cnn_struct=[[7, 2, 16], [7, 2, 64]]).cuda()
    B, Tq = 24, 64
    gen = torch.Generator().manual_seed(42)
    feats = torch.randn(B, 64, Tq, generator=gen).cuda()
    c = torch.randn(B, 16, generator=gen).cuda()
    n = torch.randint(10, Tq + 1, (B,), generator=gen).cuda()
    n[0] = Tq
    wl = torch.randn(B, Tq, generator=gen).cuda()
    outs = []
    old = K.BF16_STORE[0]
    try:
        for store in (False, True):
            K.BF16_STORE[0] = store
            assert d.stores_bf16(B, 'cuda') == store
            for p in d.parameters():
                p.grad = None
            a = feats.clone().requires_grad_(True)
            cc = c.clone().requires_grad_(True)
            K.Profiler.start()
            logits = d.classify(a, n, cc)
            (logits * wl).sum().backward()
            prof = K.Profiler.stop()
            assert any(k.startswith('gemm_bf16s_kernel') for k in prof) == store, sorted(prof)
            outs.append((logits.detach().clone(), a.grad.clone(), cc.grad.clone(),
                         {k: p.grad.clone() for k, p in d.named_parameters() if p.grad is not None}))
    finally:
        K.BF16_STORE[0] = old
    (l0, ga0, gc0, p0), (l1, ga1, gc1, p1) = outs
    assert l1.dtype == torch.float32
    # (two different contracts: storage rounds the residual adds, the biLSTM output and the gradients where they are written,
    # 2^-8 relative each - the logits may differ by a few of those roundings; the same-contract bound is the oracle's job)
    close_bf16(l1, l0, 'logits', elem=3e-2, l2=1e-2)
    # gradients: a sanity bound in relative L2 only.  The two runs follow DIFFERENT rounding contracts (storage rounds dy, the
    # skip adds and the stored gradients), and a gradient with cancellation answers a 2^-8 perturbation of its terms with
    # several per cent: measured 5.4 % on d(features) here.  The same-contract check - the storage path against the oracle's
    # ``bf16_mode(store=True)`` - is what test_networks_bf16_vs_rounded_oracle / the C3 full-batch test hold at 2e-2.
    close_bf16(ga1, ga0, 'd features', elem=1.0, l2=0.15)
    close_bf16(gc1, gc0, 'd c', elem=1.0, l2=0.15)
    assert set(p0) == set(p1)
    for k in p0:
        if k.split('.')[-1].startswith('bias') and k.endswith('_v'):
            continue
        close_bf16(p1[k], p0[k], k, elem=1.0, l2=0.15)


def test_lstm_bf16_storage_reads_the_current_weights_after_every_update(K, bf16):
    """LSTMSeqFn on bf16 storage at the smallest shape the persistent launches take (H 64: grids of 16 and 4 workgroups), six
    iterations, ragged lengths.  Run A keeps ONE set of Parameters and overwrites all of them with fresh values before every
    iteration; run B builds new Parameters from clones of the same values, so no kept bf16 image of W_ih can serve it.  A
    stale image (of the previous iteration's weights, 0.1-scale noise replaced by other 0.1-scale noise) is a gross error,
    not a rounding one: y, dx and every parameter gradient must be EQUAL."""
    from audiogan_amd import ops
    T, B, Fx, H, ndir = 6, 8, 64, 64, 2
    dev = torch.device('cuda')
    assert K.lstm_step_ok(B, H) and K.lstm_persist_ok(B, H, ndir, dev) and K.lstm_persist_bwd_ok(B, H, ndir, dev)
    gen = torch.Generator().manual_seed(91)
    lens = torch.tensor([6, 3, 5, 1, 6, 2, 4, 5]).cuda()
    shapes = [(4 * H, Fx), (4 * H, H), (4 * H,), (4 * H,)] * ndir
    kept = [torch.nn.Parameter(torch.zeros(s).cuda()) for s in shapes]
    for it in range(6):
        vals = [(torch.randn(s, generator=gen) * 0.1).cuda() for s in shapes]
        x = torch.randn(T, B, Fx, generator=gen).cuda().to(torch.bfloat16)
        gy = torch.randn(T, B, ndir * H, generator=gen).cuda().to(torch.bfloat16)
        with torch.no_grad():
            for p, v in zip(kept, vals):
                p.copy_(v)
        got = []
        for w in (kept, [torch.nn.Parameter(v.clone()) for v in vals]):
            for p in w:
                p.grad = None
            xx = x.clone().requires_grad_(True)
            y = ops.LSTMSeqFn.apply(xx, lens, ndir, None, *w)
            y.backward(gy)
            got.append([y.detach(), xx.grad] + [p.grad for p in w])
        assert K.lstm_persist_status() == 0
        assert got[0][0].dtype == torch.bfloat16 and got[0][1].dtype == torch.bfloat16 and float(got[0][0].abs().max()) > 0
        for i, (a, b) in enumerate(zip(*got)):
            assert torch.equal(a, b), (it, i, float((a.float() - b.float()).abs().max()))
