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
