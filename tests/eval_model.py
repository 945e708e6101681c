"""Torch-CPU models of the evaluation kernels of ``audiogan_amd.kernels`` (ag_ltas_power, ag_score_accum; contracts in
include/audiogan_hip.h), their float64 restatements and the shared test inputs  --  TEST INFRASTRUCTURE, installed after
``kernel_model.install``."""
import numpy as np
import torch

FRAME, HOP, BINS = 256, 128, 129
# |P - P64| <= LTAS_BOUND * max_k P64[b] per clip (set by the issue): a sequential fp32 restatement stays under 1e-6 on the
# test inputs, a dropped or doubled sample moves a bin by about 4e-3
LTAS_BOUND = 2e-5
_I = np.arange(FRAME, dtype=np.float64)
_WIN64 = 0.5 - 0.5 * np.cos(2.0 * np.pi * _I / FRAME)
_ANG = 2.0 * np.pi * np.outer(_I, np.arange(BINS, dtype=np.float64)) / FRAME
# window and twiddles: float64 values rounded once to fp32
_WIN32 = torch.from_numpy(_WIN64.astype(np.float32))
_COS32, _SIN32 = torch.from_numpy(np.cos(_ANG).astype(np.float32)), torch.from_numpy(np.sin(_ANG).astype(np.float32))


def frame_count(n):
    return (n - FRAME) // HOP + 1 if n >= FRAME else 1


def _frames(row, n, dtype):
    """[frames, 256]: the clip's frames, reading nothing at or past n"""
    nf = frame_count(n)
    out = torch.zeros(nf, FRAME, dtype=dtype)
    if n >= FRAME:
        for j in range(nf):
            out[j] = row[j * HOP:j * HOP + FRAME]
    else:
        out[0, :n] = row[:n]
    return out


def ltas_power(x, lens, out=None, nframes=None):
    assert x.dtype == torch.float32 and x.dim() == 2 and (x.size(1) == 1 or x.stride(1) == 1)
    B, L = x.shape
    if out is None:
        out = torch.empty(B, BINS)
    assert tuple(out.shape) == (B, BINS) and out.dtype == torch.float32
    for b in range(B):
        n = L if lens is None else max(0, min(int(lens[b]), L))
        f = _frames(x[b].detach(), n, torch.float32) * _WIN32
        re, im = f @ _COS32, f @ _SIN32
        out[b] = (re * re + im * im).sum(0) / float(f.size(0))
        if nframes is not None:
            assert nframes.dtype == torch.int32
            nframes[b] = f.size(0)
    return out


def ltas_power64(x, lens):
    """float64 numpy: (P [B, 129], frame counts); reads nothing at or past the lengths"""
    x = np.asarray(x)
    B, L = x.shape
    P, nf = np.zeros((B, BINS)), np.zeros(B, dtype=np.int64)
    for b in range(B):
        n = L if lens is None else max(0, min(int(lens[b]), L))
        f = _frames(torch.from_numpy(np.ascontiguousarray(x[b])).double(), n, torch.float64).numpy() * _WIN64
        P[b] = (np.abs(np.fft.rfft(f, axis=1)) ** 2).mean(0)
        nf[b] = f.shape[0]
    return P, nf


def score_accum(cls, nframes, target, positive, acc):
    assert cls.dtype == torch.float32 and cls.dim() == 2 and acc.dtype == torch.float64 and acc.numel() == 6
    B, T = cls.shape
    tg = torch.tensor(float(target), dtype=torch.float32)
    add = [0.0] * 6
    for b in range(B):
        n = T if nframes is None else max(0, min(int(nframes[b]), T))
        if n < 1:
            continue
        v = cls[b, :n].detach()
        m = (-v).clamp(min=0)
        per = v - v * tg + m + ((-m).exp() + (-v - m).exp()).log()          # fp32 per element (audiogan.py:191-192)
        vd = v.double()
        add[0] += 1.0
        add[1] += float(per.double().sum()) / n
        add[2] += float(n)
        add[3] += float(((v > 0) if positive else (v < 0)).sum())
        add[4] += float(vd.sum())
        add[5] += float((vd * vd).sum())
    acc += torch.tensor(add, dtype=torch.float64)
    return acc


def score_accum64(x, nframes, target, positive):
    """float64 numpy: the six words one call adds; reads nothing outside the lengths"""
    x = np.asarray(x)
    B, T = x.shape
    a = np.zeros(6)
    for b in range(B):
        n = max(0, min(int(nframes[b]), T))
        if n < 1:
            continue
        v = x[b, :n].astype(np.float64)
        m = np.maximum(-v, 0.0)
        per = v - v * float(target) + m + np.log(np.exp(-m) + np.exp(-v - m))
        a += [1.0, per.sum() / n, n, ((v > 0) if positive else (v < 0)).sum(), v.sum(), (v * v).sum()]
    return a


# ---- the shapes of the two GPU kernel tests (the CPU tests run the models on the same ones) ---------------------------
LTAS_L, LTAS_LD = 1024, 1031
LTAS_LENS = (1024, 700, 384, 383, 256, 100)          # 7, 4, 2, 1 and 1 frames, and one zero-padded frame
LTAS_FRAMES = (7, 4, 2, 1, 1, 1)
LTAS_KINDS = ('randn', 'sine', 'walk')


def ltas_case(kind, L=LTAS_L, ld=LTAS_LD, lens=LTAS_LENS, seed=0):
    """-> (buf [B, ld] float32 with NaN at every position at or past each length - padding columns included - whose
    [:, :L] view is the kernel's input, lens int64)"""
    rs = np.random.RandomState(seed)
    B = len(lens)
    t = np.arange(L, dtype=np.float64)
    if kind == 'randn':
        x = rs.randn(B, L) * 0.3
    elif kind == 'sine':
        bins = rs.randint(3, 120, size=(B, 1))           # bin-centred: an integer number of periods per frame
        x = 0.5 * np.sin(2.0 * np.pi * bins * t[None, :] / FRAME + rs.rand(B, 1)) + 1e-3 * rs.randn(B, L)
    else:
        x = np.cumsum(rs.randn(B, L) * 0.05, axis=1)
    buf = np.full((B, ld), np.nan, dtype=np.float32)
    for b, n in enumerate(lens):
        buf[b, :n] = x[b, :n]
    return torch.from_numpy(buf), torch.tensor(lens, dtype=torch.int64)


SCORE_NF = (7, 1, 3, 9, 2)          # T = 7: the 9 clamps


def score_case(seed=0, B=5, T=7, nf=SCORE_NF):
    """-> (logits [B, T] float32 with NaN in every masked entry, nframes int64)"""
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, T) * 1.5).astype(np.float32)
    for b, n in enumerate(nf):
        x[b, min(n, T):] = np.nan
    return torch.from_numpy(x), torch.tensor(nf, dtype=torch.int64)


def check_ltas(P, nframes, buf, lens, L, frames=None):
    """the issue's bound, clip by clip; prints the worst ratio"""
    P64, nf64 = ltas_power64(buf[:, :L].numpy(), lens.numpy())
    got = P.detach().cpu().double().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - P64).max(1) / np.maximum(P64.max(1), 1e-300)          # (an empty clip: exactly zero)
    print('ltas_power: worst |P - P64| / max_k P64 per clip: %s (bound %g)' % (np.array2string(err, precision=2), LTAS_BOUND))
    assert (err <= LTAS_BOUND).all(), err
    if nframes is not None:
        assert nframes.cpu().tolist() == nf64.tolist(), (nframes.cpu().tolist(), nf64.tolist())
    if frames is not None:
        assert nf64.tolist() == list(frames)


def check_scores(acc, want):
    """words 0, 2, 3 exact; word 1 within 1e-6 relative (fp32 softplus terms, all positive, summed in double); words 4 and 5
    within 1e-12 relative (fp32 values summed in double)"""
    got = acc.detach().cpu().numpy()
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print('score_accum: got %s\n             want %s\n             rel %s' % (got, want, np.array2string(rel, precision=2)))
    assert got[0] == want[0] and got[2] == want[2] and got[3] == want[3], (got, want)
    assert rel[1] <= 1e-6, rel
    assert rel[4] <= 1e-12 and rel[5] <= 1e-12, rel


ALL = ('ltas_power', 'score_accum')


def install(monkeypatch):
    """after ``kernel_model.install(monkeypatch)``: the evaluation kernels' CPU models"""
    import audiogan_amd.kernels as K
    for n in ALL:
        assert hasattr(K, n), 'eval model has %s but audiogan_amd.kernels does not' % n
        monkeypatch.setattr(K, n, globals()[n])
