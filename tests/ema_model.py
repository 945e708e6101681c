"""Torch-CPU model of ``audiogan_amd.kernels.ema_update`` (ag_ema_update; contract in include/audiogan_hip.h) and the float64
recursion the EMA tests compare against  --  TEST INFRASTRUCTURE, installed after ``kernel_model.install``."""
import numpy as np
import torch

ULP = 2.0 ** -24
STEP_BOUND = 5 * ULP       # per update and element, times max(|p|, |e|): three fp32 roundings (difference 2, product 2 if
#                            the compiler does not fuse it, sum 1)


def weight(decay, warmup, k):
    """1 - d as the kernel forms it: every operation rounded to fp32"""
    d = np.float32(decay)
    if warmup:
        kf = np.float32(max(0, int(k)))
        d = min(d, (np.float32(1) + kf) / (np.float32(10) + kf))
    return np.float32(1) - d


def lerp64(e64, p, w):
    """one update in float64 with the kernel's fp32 weight"""
    return e64 + float(w) * (p.detach().double() - e64)


def ema_plan(shadows, params):
    """(the model needs no launch plan)"""
    assert len(shadows) == len(params) and len(params) > 0
    return None


def ema_update(shadows, params, decay, warmup, step_dev, step0, k=0, plan=None):
    if not 0.0 <= float(decay) <= 1.0:
        raise ValueError('audiogan_amd: ema_update needs 0 <= decay <= 1, got %r' % (decay,))
    assert len(shadows) == len(params) and len(params) > 0
    if step_dev is not None:
        assert step_dev.dtype == torch.int32
        k = int(step_dev.reshape(-1)[0].item()) - int(step0)
    w = weight(decay, warmup, k)
    for e, p in zip(shadows, params):
        assert e.dtype == p.dtype == torch.float32 and e.is_contiguous() and p.is_contiguous() and e.numel() == p.numel() >= 1
        pf = p.detach().reshape(-1)
        if w == 1:
            e.copy_(pf)
        else:
            # fmaf(w, fl(p - e), e): the product of two fp32 values is exact in float64
            e.copy_((e.double() + float(w) * (pf - e).double()).float())


ALL = ('ema_plan', 'ema_update')


def install(monkeypatch):
    """after ``kernel_model.install(monkeypatch)``: the EMA kernel's CPU model"""
    import audiogan_amd.kernels as K
    for n in ALL:
        assert hasattr(K, n), 'ema model has %s but audiogan_amd.kernels does not' % n
        monkeypatch.setattr(K, n, globals()[n])
