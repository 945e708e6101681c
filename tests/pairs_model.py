"""Torch-CPU model of ``audiogan_amd.kernels.dtw_pairs`` (ag_dtw_pairs; contract in include/audiogan_hip.h), its checker against
float64, the mutants the checker must reject, the case tables of the GPU tests and the synthetic words of the crossed
evaluation  --  TEST INFRASTRUCTURE, installed after ``align_model.install``.

The model is the contract's own sentence: gather the two sequences of every pair, then ``align_model.dtw_cost``.  Bounds are
those of tests/align_model.py: integer inputs bit for bit, real inputs within ``dtw_real_bound`` of ``dtw64``, pair by pair."""
import numpy as np
import torch

from tests import align_model
from tests.align_model import CEPW, GUARD, GUARD_VALUE, dtw64, dtw_case, dtw_real_bound, guarded

MUTANTS = ('transposed', 'nfb_at_ia', 'off_by_one', 'other_capacity')


def pair_lists(Na, Nb, ia=None, ib=None, clamp=True):
    """-> (I, J) int64 numpy: the sequences of every pair, in output order (NULL lists: the cross product, row-major)"""
    if ia is None:
        I, J = np.repeat(np.arange(Na), Nb), np.tile(np.arange(Nb), Na)
    else:
        I, J = np.asarray(ia, dtype=np.int64), np.asarray(ib, dtype=np.int64)
    return (np.clip(I, 0, Na - 1), np.clip(J, 0, Nb - 1)) if clamp else (I, J)


def dtw_pairs(cep_a, nf_a, cep_b, nf_b, ia=None, ib=None, out=None, mutate=None):
    assert cep_a.dtype == cep_b.dtype == torch.float32 and cep_a.dim() == cep_b.dim() == 3
    assert cep_a.size(2) == cep_b.size(2) == CEPW and (ia is None) == (ib is None)
    Na, Fa, Nb, Fb = cep_a.size(0), cep_a.size(1), cep_b.size(0), cep_b.size(1)
    assert nf_a is None or (nf_a.dtype == torch.int32 and nf_a.numel() == Na)
    assert nf_b is None or (nf_b.dtype == torch.int32 and nf_b.numel() == Nb)
    if ia is not None:
        assert ia.dtype == ib.dtype == torch.int32 and ia.dim() == 1 and ia.shape == ib.shape
    I, J = pair_lists(Na, Nb, None if ia is None else ia.numpy(), None if ib is None else ib.numpy(), clamp=False)
    if mutate == 'off_by_one':
        I, J = I + 1, J + 1
    I, J = np.clip(I, 0, Na - 1), np.clip(J, 0, Nb - 1)          # the kernel's clamp: a wrong index is a wrong pair
    shape = (Na, Nb) if ia is None else (len(I),)
    if out is None:
        out = torch.empty(shape)
    assert tuple(out.shape) == shape and out.dtype == torch.float32
    na = torch.full((Na,), Fa, dtype=torch.int32) if nf_a is None else nf_a
    nb = torch.full((Nb,), Fb, dtype=torch.int32) if nf_b is None else nf_b
    ga, gb = cep_a[torch.from_numpy(I)], cep_b[torch.from_numpy(J)]
    ca, cb = na[torch.from_numpy(I)], nb[torch.from_numpy(np.clip(I, 0, Nb - 1) if mutate == 'nfb_at_ia' else J)]
    if mutate == 'other_capacity':
        ca, cb = ca.clamp(max=Fb), cb.clamp(max=Fa)
    flat = align_model.dtw_cost(ga, ca, gb, cb)
    if mutate == 'transposed' and ia is None:
        flat = flat.view(Na, Nb).t().contiguous().view(-1)          # pair (i, j) lands at [j * Na + i]
    out.view(-1).copy_(flat)
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------
def bank(counts, F, integer, seed):
    """-> (cep [N, F, 16], nf [N]) from ``align_model.dtw_case``: NaN in rows past the counts and in columns 0 and 13..15"""
    c, n, _, _ = dtw_case(tuple((k, 1) for k in counts), F, 1, integer, seed=seed)
    return c, n


# the rectangular cross product every mutant shows on: unequal counts, some above the other side's capacity
RECT = dict(counts_a=(9, 20, 1, 14, 17), Fa=20, counts_b=(12, 3, 7, 1, 11, 5, 10), Fb=12)
# wave form (GPU): the counts at capacity 64 a side - one lane, two, a few, half a wave and a lane, the last lane idle, full
WAVE_COUNTS = (1, 2, 7, 33, 63, 64)
LISTS = {1: ((3,), (2,)), 4: ((0, 5, 5, 2), (1, 1, 4, 0)), 5: ((4, 4, 0, 3, 1), (5, 5, 2, 0, 3))}          # P -> (ia, ib), repeats


def rect_case(integer, seed=0):
    ca, na = bank(RECT['counts_a'], RECT['Fa'], integer, seed)
    cb, nb = bank(RECT['counts_b'], RECT['Fb'], integer, seed + 100)
    return ca, na, cb, nb


def run_guarded(fn, ca, na, cb, nb, ia=None, ib=None, on=lambda t: t):
    """-> the output on the CPU (flat, in pair order), NaN-filled between intact guard floats before the call"""
    P = ca.size(0) * cb.size(0) if ia is None else len(ia)
    flat, out = guarded((ca.size(0), cb.size(0)) if ia is None else (P,), on=on)
    kw = {} if ia is None else dict(ia=on(torch.tensor(ia, dtype=torch.int32)), ib=on(torch.tensor(ib, dtype=torch.int32)))
    assert fn(on(ca), None if na is None else on(na), on(cb), None if nb is None else on(nb), out=out, **kw) is out
    f = flat.detach().cpu()
    assert (f[:GUARD] == GUARD_VALUE).all() and (f[-GUARD:] == GUARD_VALUE).all()
    return out.detach().cpu().reshape(-1)


def check_pairs(fn, ca, na, cb, nb, ia=None, ib=None, integer=False, on=lambda t: t):
    """``fn`` on one case against ``dtw64`` of the gathered pairs: integer inputs exactly, real ones within the bound"""
    I, J = pair_lists(ca.size(0), cb.size(0), ia, ib)
    n, m = na.numpy()[I], nb.numpy()[J]
    want = dtw64(ca.numpy()[I], n, cb.numpy()[J], m)
    got = run_guarded(fn, ca, na, cb, nb, ia, ib, on=on).double().numpy()
    if integer:
        assert (want == np.round(want)).all() and want.max() < 2 ** 24
        assert np.array_equal(got, want), (got, want)
        return 0.0
    bound = np.array([dtw_real_bound(a, b, w) for a, b, w in zip(n, m, want)])
    assert np.isfinite(got).all() and (np.abs(got - want) <= bound).all(), (got, want)
    return float((np.abs(got - want) / bound).max())


def paired_adaptor(fn, F=None):
    """``dtw_cost``'s signature on ``dtw_pairs``: ia = ib = arange.  ``F``: the pairs whose two counts fit into F frames go
    through banks cut to that capacity (the shared checkers' cases at a capacity the wave form takes), the others as they
    are; ``run.cut`` counts the pairs that took the cut banks"""
    def one(ca, na, cb, nb, out=None):
        idx = torch.arange(ca.size(0), dtype=torch.int32, device=ca.device)
        return fn(ca, na, cb, nb, ia=idx, ib=idx, out=out)

    def run(ca, na, cb, nb, out):
        if F is None:
            return one(ca, na, cb, nb, out=out)
        fit = (na <= F) & (nb <= F)
        run.cut += int(fit.sum())
        if bool(fit.any()):
            out[fit] = one(ca[fit][:, :F].contiguous(), na[fit], cb[fit][:, :F].contiguous(), nb[fit])
        if not bool(fit.all()):
            out[~fit] = one(ca[~fit], na[~fit], cb[~fit], nb[~fit])
        return out
    run.cut = 0
    return run


# ---- the synthetic words of the issue ------------------------------------------------------------------------------------------
WORDS = ((400, 1800), (1800, 400), (700, 2500), (2500, 700), (1200, 3000), (300, 1000), (1000, 300), (3000, 1200))
WORD_N, WORD_SR = 4096, 8000.0
REAL_LENS = (4096, 3500, 4096, 3000, 3800, 4096, 2900, 4096)
FAKE_LENS = (3700, 4096, 3100, 4096, 4096, 3300, 4096, 3600)


def take(w, s, seed, length):
    """float32 [4096]: word w at amplitude 0.5, f1 until the fraction s of the clip and f2 after it, 1e-3 noise, zero at and
    past ``length``"""
    f1, f2 = WORDS[w]
    t = np.arange(WORD_N, dtype=np.float64) / WORD_SR
    k = int(round(s * WORD_N))
    x = 0.5 * np.where(np.arange(WORD_N) < k, np.sin(2 * np.pi * f1 * t), np.sin(2 * np.pi * f2 * t))
    x = x + 1e-3 * np.random.RandomState(seed).randn(WORD_N)
    x[length:] = 0.0
    return torch.from_numpy(x.astype(np.float32))


def word_sets():
    """-> (reals, real_len, fakes, fake_len, seconds): [8, 4096] fp32 each, int64 lengths; the second takes have the fakes'"""
    reals = torch.stack([take(w, 0.5, 10 + w, n) for w, n in enumerate(REAL_LENS)])
    fakes = torch.stack([take(w, 0.405, 30 + w, n) for w, n in enumerate(FAKE_LENS)])
    seconds = torch.stack([take(w, 0.595, 50 + w, n) for w, n in enumerate(FAKE_LENS)])
    return reals, torch.tensor(REAL_LENS), fakes, torch.tensor(FAKE_LENS), seconds


def check_words(matrix_fn, scores_fn, on=lambda t: t):
    """the conditions of the issue (they separate the cases; they are not accuracy bounds): honest fakes retrieve their word
    with a margin of 3, a word-blind generator loses word_hit and cover_db and keeps nn_db, two takes of a word are more
    than 5 dB apart and a take is at exactly 0 from itself"""
    reals, rl, fakes, fl, seconds = (on(t) for t in word_sets())
    W = len(WORDS)
    same = torch.eye(W, dtype=torch.bool)
    M = matrix_fn(fakes, fl, reals, rl).cpu()
    assert M.dtype == torch.float64 and tuple(M.shape) == (W, W)
    honest = scores_fn(M, same)
    off = M.masked_fill(same, float('inf')).min(1).values
    print('honest fakes: %s; off-diagonal minimum / diagonal %s' % (honest, (off / M.diagonal()).tolist()))
    assert honest['word_hit'] == 1.0 and honest['chance'] == 1.0 / W
    assert (off >= 3.0 * M.diagonal()).all()
    blind = scores_fn(matrix_fn(fakes[:1].repeat(W, 1), fl[:1].repeat(W), reals, rl).cpu(), same)
    print('word-blind fakes: %s' % (blind,))
    assert blind['word_hit'] == 0.125
    assert blind['cover_db'] >= 5.0 * honest['cover_db'] and blind['nn_db'] < 2.0 * honest['nn_db']
    again = matrix_fn(fakes, fl, seconds, fl).cpu().diagonal()
    itself = matrix_fn(fakes, fl, fakes, fl).cpu().diagonal()
    print('take against second take: %s dB' % (again.tolist(),))
    assert (again > 5.0).all() and (itself == 0.0).all()
    return honest, blind


ALL = ('dtw_pairs',)


def install(monkeypatch):
    """after ``align_model.install``: the CPU model of the all-pairs launch"""
    import audiogan_amd.kernels as K
    for n in ALL:
        assert hasattr(K, n), 'pairs model has %s but audiogan_amd.kernels does not' % n
        monkeypatch.setattr(K, n, globals()[n])
