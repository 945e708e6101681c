"""Torch-CPU models of the summary kernels of ``audiogan_amd.kernels`` (ag_logit_summary, ag_sqnorm_rows, ag_vec_stats,
ag_summary_commit; contracts in include/audiogan_hip.h)  --  TEST INFRASTRUCTURE, installed after ``kernel_model.install``."""
import struct

import torch

COLS = 16


def logit_summary(cls, nframes, positive, out=None):
    B, T = cls.shape
    x = cls.detach().double()
    n = nframes if nframes is not None else torch.full((B,), T, dtype=torch.long)
    mask = torch.arange(T).view(1, T) < n.view(B, 1)
    hit = ((x > 0) if positive else (x < 0)) & mask
    mean = x.mean()
    std = ((x - mean) ** 2).mean().sqrt()
    h, c = hit.sum().float(), mask.sum().float()
    r = torch.stack([mean.float(), std.float(), h, c, h / c])
    if out is None:
        return r
    out.copy_(r)
    return out


def sqnorm_rows(gx, nframes, scale, part=None, out=None, finish=True):
    B, L = gx.shape
    n = nframes.double() if nframes is not None else torch.full((B,), float(L), dtype=torch.float64)
    p = (float(scale) * (gx.detach().float() ** 2).double().sum(1) / n).float()
    if part is None:
        part = torch.empty(B)
    part.copy_(p)
    if finish:
        if out is None:
            out = torch.empty(1)
        out.copy_((part.double().sum() / B).float().view(1))
    return part, (out if finish else None)


def vec_stats(v, sign=1.0, out=None):
    x = v.detach().double()
    mean = x.mean()
    r = torch.stack([(float(sign) * mean).float(), ((x - mean) ** 2).mean().sqrt().float()])
    if out is None:
        return r
    out.copy_(r)
    return out


def summary_commit(ring, cursor, cols, part=None, part_col=-1):
    assert ring.dtype == torch.int32 and tuple(ring.shape[1:]) == (COLS,) and cursor.dtype == torch.int32 and len(cols) == COLS
    row, seq = int(cursor[0]), int(cursor[1])
    words = []
    for i, c in enumerate(cols):
        if i == 1:
            w = seq
        elif part is not None and i == part_col:
            w = (part.double().sum() / part.numel()).float().view(1).view(torch.int32).item()
        elif torch.is_tensor(c):
            assert c.numel() == 1 and c.dtype in (torch.float32, torch.int32), (i, c.dtype, tuple(c.shape))
            w = c.detach().reshape(1).clone().view(torch.int32).item()
        elif isinstance(c, float):
            w = struct.unpack('<i', struct.pack('<f', c))[0]
        elif c is None:
            w = 0
        else:
            w = struct.unpack('<i', struct.pack('<I', int(c) & 0xFFFFFFFF))[0]
        words.append(w)
    ring[row] = torch.tensor(words, dtype=torch.int32)
    cursor[0] = (row + 1) % ring.size(0)
    cursor[1] = seq + 1


ALL = ('logit_summary', 'sqnorm_rows', 'vec_stats', 'summary_commit')


def install(monkeypatch):
    """after ``kernel_model.install(monkeypatch)``: the summary kernels' CPU models"""
    import audiogan_amd.kernels as K
    for n in ALL:
        assert hasattr(K, n), 'summary model has %s but audiogan_amd.kernels does not' % n
        monkeypatch.setattr(K, n, globals()[n])
