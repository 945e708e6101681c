"""K.Profiler files a call under the name the library reports for the kernel it launched (ag_last_kernel): the names below
come from reading the C dispatch (gemm.hip, conv_engine.hip, conv_engine_impl.h, conv_c1.hip, conv_grad.hip) at these
shapes, in rocprofv3's spelling."""
import pytest
import torch

from tests.test_gpu_kernels import D_LAYERS, _mk, _out_len

pytestmark = pytest.mark.gpu

D1, D5 = D_LAYERS[0], D_LAYERS[4]
B = 64


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    return K_


def _conv_fwd(K, layer):
    """-> a closure that runs the layer's forward conv once (batch 64)"""
    kind, cin, cout, k, s, p, lin = layer
    w, x = _mk(kind, cin, cout, k, s, p, lin, B, 11)
    wpa, wpb = torch.zeros(K.wpa_numel(cout, cin, k)).cuda(), torch.zeros(K.wpb_numel(cout, cin, k, s)).cuda()
    K.prep_conv_weight(w.cuda(), wpa, wpb, s)
    x = x.cuda()
    y = torch.empty(B, cout, _out_len(kind, lin, k, s, p)).cuda()
    return lambda: K.conv_engine(x, wpa, y, k, s, p, 0)


def _conv_wgrad(K, layer):
    kind, cin, cout, k, s, p, lin = layer
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(B, cin, lin, generator=gen).cuda()
    gy = torch.randn(B, cout, _out_len(kind, lin, k, s, p), generator=gen).cuda()
    dw = torch.zeros(cout, cin, k).cuda()
    return lambda: K.conv_wgrad(gy, x, dw, k, s, p)


def _gemm(K):
    """[16384 x 1024] = [16384 x 1024] . [1024 x 1024]^T (the shape of DESIGN 4.3's table)"""
    gen = torch.Generator().manual_seed(13)
    a, w = torch.randn(16384, 1024, generator=gen).cuda(), torch.randn(1024, 1024, generator=gen).cuda()
    c = torch.empty(16384, 1024).cuda()
    return lambda: K.gemm(a, w, c, tb=True)


def _names(K, call, mode='f32'):
    with K.precision(mode):
        K.Profiler.start()
        try:
            call()
        finally:
            prof = K.Profiler.stop()
    assert all(r['n'] == 1 for r in prof.values()), prof
    return sorted(prof)


def test_half_width_conv_tiles_are_named(K):
    assert _names(K, _conv_fwd(K, D5)) == ['conv_engine_kernel<2,1,2,2,7,2>']


def test_single_channel_conv_kernels_are_named(K):
    assert _names(K, _conv_fwd(K, D1)) == ['conv_c1_fwd_kernel<2,7,4>']
    assert _names(K, _conv_wgrad(K, D1)) == ['conv_c1_wgrad4_kernel<2,7,8>']


def test_bf16_conv_kernels_are_named(K):
    (fwd,) = _names(K, _conv_fwd(K, D5), 'bf16')
    assert fwd.startswith('conv_engine_bf16_kernel<') and fwd.endswith('>') and fwd.count(',') == 4, fwd
    (wg,) = _names(K, _conv_wgrad(K, D5), 'bf16')
    assert wg.startswith('conv_wgrad_bf16_kernel<'), wg


def test_gemm_tile_and_bf16_gemm_are_named(K):
    call = _gemm(K)
    assert _names(K, call) == ['gemm_tile_kernel<0,1,256,256,2,4>']
    assert _names(K, call, 'bf16') == ['gemm_bf16_kernel<0,1,0>']


def test_only_times_the_one_kernel_after_a_discovery_pass(K):
    conv, gemm = _conv_fwd(K, D5), _gemm(K)
    K.Profiler.start()
    conv()
    gemm()
    disc = K.Profiler.stop()
    (name,) = [k for k in disc if k.startswith('conv_')]
    assert len(disc) == 2
    K.Profiler.start(only=name)
    conv()
    gemm()
    prof = K.Profiler.stop()
    assert sorted(prof) == [name] and prof[name]['n'] == 1, prof


def _records(K, call):
    """{key: launches} of one profiled call"""
    K.Profiler.start()
    try:
        call()
    finally:
        prof = K.Profiler.stop()
    return {k: r['n'] for k, r in prof.items()}


def _lstm_layer(K, H, T=3, B=4, ndir=2):
    """a forward pass of a bidirectional layer on the per-step kernels -> the closures of one more forward and of its backward"""
    gen = torch.Generator().manual_seed(14)
    mk = lambda *shp: [(torch.randn(*shp, generator=gen) * 0.3).cuda() for _ in range(ndir)]      # noqa: E731
    pre0, whh = mk(T, B, 4 * H), mk(4 * H, H)
    c_all = [torch.zeros(T + 1, B, H).cuda() for _ in range(ndir)]
    hbuf = [torch.empty(2, B, H).cuda() for _ in range(ndir)]
    y, dy = torch.empty(T, B, ndir * H).cuda(), torch.randn(T, B, ndir * H, generator=gen).cuda()
    gates = [p.clone() for p in pre0]
    dgates = [torch.empty(T, B, 4 * H).cuda() for _ in range(ndir)]
    dhb, dcb = ([torch.empty(2, B, H).cuda() for _ in range(ndir)] for _ in range(2))

    def fwd():
        for g, p in zip(gates, pre0):
            g.copy_(p)
        K.lstm_seq_fwd(gates, whh, c_all, hbuf, y, None)
    fwd()
    return fwd, lambda: K.lstm_seq_bwd(gates, whh, c_all, dy, dgates, dhb, dcb, None)


def test_per_step_recurrent_launches_are_filed_per_kernel(K):
    """with the persistent launches off a layer pass is T launches: the keys and counts lstm_seq_fwd / lstm_seq_bwd and the
    _work_seq_* models give at T = 3 - the fused step kernels at H % 16 == 0, cell backward + skinny product otherwise"""
    old = K.PERSIST[0]
    K.PERSIST[0] = False
    try:
        with K.precision('f32'):
            fwd, bwd = _lstm_layer(K, 16)
            assert _records(K, fwd) == {'lstm_step_fwd_kernel': 3}
            assert _records(K, bwd) == {'lstm_step_bwd_kernel': 3}
            fwd, bwd = _lstm_layer(K, 8)
            assert _records(K, bwd) == {'lstm_cell_bwd2_kernel': 3, 'skinny_gemm_kernel': 2}
        torch.cuda.synchronize()
    finally:
        K.PERSIST[0] = old


def test_a_wrapper_without_a_model_is_filed_under_its_name_and_a_named_one_under_the_kernels(K):
    x = torch.randn(4).cuda()
    y = torch.empty(4).cuda()
    assert _records(K, lambda: K.act_fwd(x, y, K.ACT_TANH)) == {'act_fwd': 1}
    v = torch.randn(8).cuda()
    last = []
    got = _records(K, lambda: (K.vec_stats(v), last.append(K.lib.ag_last_kernel().decode())))
    assert got == {last[0]: 1} and last[0] != 'vec_stats', (got, last)
    torch.cuda.synchronize()
