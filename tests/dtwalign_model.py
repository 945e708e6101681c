"""Torch-CPU fp32 model of ``audiogan_amd.kernels.dtw_align`` (ag_dtw_align; contract in include/audiogan_hip.h), the case table,
the checkers against ``audiogan_amd.align.path64`` and against the definition of a path, the mutants the checkers must reject,
and the synthetic utterances of the alignment tests  --  TEST INFRASTRUCTURE, installed after ``pairs_model.install``.

Bounds.
  integer cases   ONE non-zero column (column 1) of small integers: every local cost |delta| is an integer, every sum is
                  exact in fp32 and in float64, so total, lo and hi are EQUAL to path64's - ties, of which such inputs are
                  full, included.
  real cases      the total is bit-equal to dtw_cost's (on the GPU; the model's is the model of dtw_cost's); the path that
                  was RETURNED, its cost re-added in float64, exceeds path64's optimum by at most
                  align_model.dtw_real_bound(n, m, D64): near-ties may pick another path of that cost.
  boundaries      the utterances below: see ``BOUNDARY`` at the end of this file."""
import numpy as np
import torch

from audiogan_amd import align
from tests import align_model
from tests.align_model import CEPW, DTW_MAX, GUARD, GUARD_VALUE, dtw_real_bound, guarded, local_cost

DIAG, UP, LEFT = 0, 1, 2
MUTANTS = ('tie_swapped', 'lohi_off_by_one', 'diag1', 'unclamped')


# ----------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------
def _path32(d, order=(DIAG, UP, LEFT), diag_weight=2.0, off=0):
    """the recursion over a local-cost matrix d [n, m] in fp32, one anti-diagonal at a time, and the walk back -> (total, lo,
    hi).  The mutants' handles: ``order`` - which predecessor wins a tie, first to last; ``diag_weight``; ``off`` - added to
    the row the walk notes when it leaves a column"""
    n, m = d.shape
    D = np.full((n + 1, m + 1), np.inf, dtype=np.float32)          # D[i + 1, j + 1] = D(i, j)
    code = np.full((n, m), LEFT, dtype=np.uint8)
    order = np.array(order, dtype=np.uint8)
    D[1, 1] = d[0, 0] + d[0, 0]
    for s in range(1, n + m - 1):
        i = np.arange(max(0, s - m + 1), min(n - 1, s) + 1)
        j = s - i
        dd = d[i, j]
        cand = {DIAG: D[i, j] + np.float32(diag_weight) * dd, UP: D[i, j + 1] + dd, LEFT: D[i + 1, j] + dd}
        cand = np.stack([cand[c] for c in order]).astype(np.float32)
        best = cand.min(0)
        D[i + 1, j + 1] = best
        code[i, j] = order[np.argmax(cand == best, axis=0)]
    code[0, :], code[:, 0] = LEFT, UP
    lo, hi = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    i, j = n - 1, m - 1
    hi[j] = i
    while i or j:
        c = code[i, j]
        if c == UP:
            i -= 1
            continue
        lo[j] = i + (off if i + off < n else 0)
        if c == DIAG:
            i -= 1
        j -= 1
        hi[j] = i
    lo[0] = 0
    return D[n, m], lo, hi


def dtw_align(cep_a, nf_a, cep_b, nf_b, total=None, lo=None, hi=None, workspace=None, mutate=None):
    """the launch's contract on CPU tensors: writes total[b] and lo / hi[b, :m] and nothing else"""
    assert cep_a.dtype == cep_b.dtype == torch.float32 and cep_a.dim() == cep_b.dim() == 3
    B, Fa, Fb = cep_a.size(0), cep_a.size(1), cep_b.size(1)
    assert cep_b.size(0) == B and cep_a.size(2) == cep_b.size(2) == CEPW and 1 <= Fa <= DTW_MAX and 1 <= Fb <= DTW_MAX
    for t in (nf_a, nf_b):
        assert t is None or (t.dtype == torch.int32 and t.numel() == B)
    total = torch.empty(B) if total is None else total
    lo = torch.empty(B, Fb, dtype=torch.int32) if lo is None else lo
    hi = torch.empty(B, Fb, dtype=torch.int32) if hi is None else hi
    assert total.dtype == torch.float32 and tuple(total.shape) == (B,)
    assert lo.dtype == hi.dtype == torch.int32 and tuple(lo.shape) == tuple(hi.shape) == (B, Fb)
    assert workspace is None or workspace.numel() * workspace.element_size() >= B * Fa * ((Fb + 15) // 16) * 4
    for b in range(B):
        n = Fa if nf_a is None else int(nf_a[b])
        m = Fb if nf_b is None else int(nf_b[b])
        if mutate == 'unclamped':
            n, m = min(n, Fa), min(m, Fb)
            if n < 1 or m < 1:          # a count of 0 taken as it is: nothing to do
                total[b] = float('inf')
                continue
        n, m = max(1, min(n, Fa)), max(1, min(m, Fb))
        d = local_cost(cep_a[b, :n].detach().numpy(), cep_b[b, :m].detach().numpy(), np.float32)
        t, l, h = _path32(d, order=(LEFT, UP, DIAG) if mutate == 'tie_swapped' else (DIAG, UP, LEFT),
                          diag_weight=1.0 if mutate == 'diag1' else 2.0, off=1 if mutate == 'lohi_off_by_one' else 0)
        total[b] = float(t)
        lo[b, :m] = torch.from_numpy(l).int()
        hi[b, :m] = torch.from_numpy(h).int()
    return total, lo, hi


def install(monkeypatch):
    """after ``pairs_model.install``: the model in place of kernels.dtw_align"""
    import audiogan_amd.kernels as K
    assert hasattr(K, 'dtw_align'), 'dtwalign model has dtw_align but audiogan_amd.kernels does not'
    monkeypatch.setattr(K, 'dtw_align', dtw_align)


# ----------------------------------------------------------------------------------------------------------------------
# cases.  A batch is a list of (n, m); capacities are the batch's.  Why each is there:
#   ROWS x COLS   rows 1, 2: no neighbour / one; 63, 64, 65: the last lane idle, a full wave, one lane of a second wave (the
#                 wave edge and its LDS hand-over); 129: three waves.  Columns 1, 15, 16, 17, 33: below, at and past one
#                 packing word of 16 decisions, and a third word.  Capacities 132 x 36: every count is BELOW capacity on
#                 both sides, so rows and columns past the counts (NaN) must stay unread and lo / hi past m unwritten.
#   EQUAL         all-zero cepstra: every cell ties three ways, so the path is the tie order and nothing else.  It is what
#                 rejects 'tie_swapped'.  (5, 3), (3, 5), (4, 4): more rows, more columns, square.
#   CLAMP         counts 0 and capacity + 3 on either side: taken as 1 and as the capacity.  Rejects 'unclamped'.
#   LIMIT         one pair of 1024 x 1024: the capacity, 64 packing words a row, 2047 steps.
# 'diag1' and 'lohi_off_by_one' are rejected by ROWS x COLS (any pair with a diagonal step off the tie-free optimum; any
# column the path leaves from a row below the last).
# ----------------------------------------------------------------------------------------------------------------------
ROWS, COLS = (1, 2, 63, 64, 65, 129), (1, 15, 16, 17, 33)
GRID = dict(pairs=tuple((n, m) for n in ROWS for m in COLS), Fa=132, Fb=36)
EQUAL = dict(pairs=((5, 3), (3, 5), (4, 4), (1, 4), (4, 1)), Fa=6, Fb=6)
CLAMP = dict(pairs=((0, 4), (9, 0), (12, 9), (0, 0)), Fa=9, Fb=6, true=((1, 4), (9, 1), (9, 6), (1, 1)))
LIMIT = dict(pairs=((1024, 1024),), Fa=1024, Fb=1024)
SMALL = dict(pairs=((1, 1), (2, 2), (7, 5), (5, 7), (17, 16), (16, 17), (33, 20)), Fa=34, Fb=21)          # the CPU's grid


def make_case(case, kind, seed=0):
    """-> (cep_a [B, Fa, 16], nf_a, cep_b [B, Fb, 16], nf_b, counts): NaN in rows past the (clamped) counts and in columns 0 and
    13..15.  ``kind``: 'integer' (column 1 holds integers in [-3, 3], columns 2..12 zero), 'equal' (all zero), 'real'"""
    rs = np.random.RandomState(seed)
    pairs, true = case['pairs'], case.get('true', case['pairs'])
    seqs = []
    for F, side in ((case['Fa'], 0), (case['Fb'], 1)):
        c = np.full((len(pairs), F, CEPW), np.nan, dtype=np.float32)
        for b, p in enumerate(true):
            k = p[side]
            v = np.zeros((k, 12), dtype=np.float32)
            if kind == 'integer':
                v[:, 0] = rs.randint(-3, 4, size=k)
            elif kind == 'real':
                v = rs.randn(k, 12).astype(np.float32)
            c[b, :k, 1:13] = v
        seqs.append(torch.from_numpy(c))
    nf_a = torch.tensor([p[0] for p in pairs], dtype=torch.int32)
    nf_b = torch.tensor([p[1] for p in pairs], dtype=torch.int32)
    return seqs[0], nf_a, seqs[1], nf_b, true


# ----------------------------------------------------------------------------------------------------------------------
# checkers
# ----------------------------------------------------------------------------------------------------------------------
def run_guarded(fn, ca, na, cb, nb, counts, on=lambda t: t, **kw):
    """-> (total, lo, hi) on the CPU.  Outputs NaN / -1 filled between guard words; afterwards the guards are intact and
    lo / hi at and past every pair's m are still -1 (columns never written, rows of other pairs untouched)"""
    B, Fb = ca.size(0), cb.size(1)
    ft, total = guarded((B,), on=on)
    fl, lo = guarded((B, Fb), dtype=torch.int32, fill=-1, on=on)
    fh, hi = guarded((B, Fb), dtype=torch.int32, fill=-1, on=on)
    got = fn(on(ca), None if na is None else on(na), on(cb), None if nb is None else on(nb), total=total, lo=lo, hi=hi, **kw)
    assert got[0] is total and got[1] is lo and got[2] is hi
    for f in (ft, fl, fh):
        f = f.detach().cpu()
        assert (f[:GUARD] == GUARD_VALUE).all() and (f[-GUARD:] == GUARD_VALUE).all()
    total, lo, hi = total.detach().cpu(), lo.detach().cpu(), hi.detach().cpu()
    for b, (n, m) in enumerate(counts):
        assert (lo[b, m:] == -1).all() and (hi[b, m:] == -1).all(), (b, n, m)
    return total, lo, hi


def check_facts(lo, hi, n, m):
    """what a path from (0, 0) to (n-1, m-1) in steps (1, 0), (0, 1), (1, 1) is, column by column"""
    lo, hi = np.asarray(lo[:m], dtype=np.int64), np.asarray(hi[:m], dtype=np.int64)
    assert lo[0] == 0 and hi[m - 1] == n - 1, (lo[0], hi[m - 1], n, m)
    assert (lo <= hi).all(), (lo, hi)
    step = lo[1:] - hi[:-1]
    assert ((step == 0) | (step == 1)).all(), (lo, hi)


def path_cost64(cep_a, cep_b, lo, hi, n, m):
    """the symmetric-pattern cost of the path (lo, hi) describes, in float64"""
    d = local_cost(np.asarray(cep_a)[:n], np.asarray(cep_b)[:m], np.float64)
    cost = 2.0 * d[0, 0]
    for j in range(m):
        if j:
            cost += (2.0 if lo[j] == hi[j - 1] + 1 else 1.0) * d[lo[j], j]
        cost += d[lo[j] + 1:hi[j] + 1, j].sum()
    return cost


def check_exact(fn, case, kind, on=lambda t: t, seed=0, **kw):
    """total, lo, hi EQUAL to path64's, and the path facts"""
    ca, na, cb, nb, counts = make_case(case, kind, seed)
    total, lo, hi = run_guarded(fn, ca, na, cb, nb, counts, on=on, **kw)
    for b, (n, m) in enumerate(counts):
        want_t, want_lo, want_hi = align.path64(ca[b].numpy(), n, cb[b].numpy(), m)
        assert want_t == round(want_t) and want_t < 2 ** 24
        assert float(total[b]) == want_t, (b, n, m, float(total[b]), want_t)
        assert np.array_equal(lo[b, :m].numpy(), want_lo), (b, n, m, lo[b, :m], want_lo)
        assert np.array_equal(hi[b, :m].numpy(), want_hi), (b, n, m, hi[b, :m], want_hi)
        check_facts(lo[b], hi[b], n, m)
    return total, lo, hi


def check_real(fn, case, on=lambda t: t, cost_fn=None, seed=1):
    """randn cepstra: the path facts; the returned path's float64 cost within dtw_real_bound of path64's optimum; with
    ``cost_fn`` (dtw_cost where ``fn`` runs) the total bit-equal to it.  -> the largest (cost - D64) / bound"""
    ca, na, cb, nb, counts = make_case(case, 'real', seed)
    total, lo, hi = run_guarded(fn, ca, na, cb, nb, counts, on=on)
    if cost_fn is not None:
        want = cost_fn(on(ca), on(na), on(cb), on(nb)).detach().cpu()
        assert torch.equal(total.view(torch.int32), want.view(torch.int32)), (total, want)
    worst = 0.0
    for b, (n, m) in enumerate(counts):
        check_facts(lo[b], hi[b], n, m)
        D64 = align.path64(ca[b].numpy(), n, cb[b].numpy(), m)[0]
        cost = path_cost64(ca[b].numpy(), cb[b].numpy(), lo[b].numpy(), hi[b].numpy(), n, m)
        bound = dtw_real_bound(n, m, D64)
        assert cost >= D64 * (1.0 - 1e-12), (b, n, m, cost, D64)          # (no path is cheaper than the optimum)
        assert cost - D64 <= bound, (b, n, m, cost, D64, bound)
        assert abs(float(total[b]) - D64) <= bound, (b, n, m, float(total[b]), D64)
        worst = max(worst, (cost - D64) / bound)
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# synthetic utterances: words are two-tone bursts (a tone that switches to another half way, as align_model.two_tone), a
# distinct pair of tones per word, 0.15 - 0.30 s at amplitude 0.5; noise 40 dB below the tones everywhere, pauses included
# ----------------------------------------------------------------------------------------------------------------------
SR = 8000
WORDS = dict(alpha=(400.0, 1800.0, 0.20), bravo=(900.0, 2600.0, 0.15), coda=(1500.0, 500.0, 0.30), delta=(2200.0, 1100.0, 0.25),
             echo=(3000.0, 700.0, 0.18), fox=(600.0, 3300.0, 0.22))
NOISE = 0.5 / np.sqrt(2.0) * 10.0 ** (-40.0 / 20.0)          # rms of a 0.5-amplitude tone, 40 dB down
LEAD_MS = 100
# (transcript, the pause after each word in ms - 0: the next word follows at once)
UTTERANCES = ((('alpha', 'bravo', 'coda'), (60, 0, 100)),
              (('delta', 'alpha', 'fox', 'echo'), (0, 400, 60, 100)),
              (('coda', 'echo', 'bravo', 'delta', 'alpha'), (400, 0, 60, 0, 100)),
              (('fox', 'coda', 'alpha', 'bravo', 'echo', 'delta'), (60, 60, 0, 400, 0, 100)))


def burst(word, scale=1.0):
    f1, f2, dur = WORDS[word]
    n = int(round(dur * scale * SR))
    t = np.arange(n) / float(SR)
    return 0.5 * np.where(np.arange(n) < n // 2, np.sin(2 * np.pi * f1 * t), np.sin(2 * np.pi * f2 * t))


def template_store():
    """word -> float32 [1, len]: one take per word, its duration changed by +20 % and -20 % in turn, noise of its own"""
    store = {}
    for k, w in enumerate(sorted(WORDS)):
        x = burst(w, 1.2 if k % 2 == 0 else 0.8)
        store[w] = (x + NOISE * np.random.RandomState(100 + k).randn(len(x))).astype(np.float32)[None, :]
    return store


def utterances():
    """-> (waves float32 [4, L] zero padded, lens, transcripts, truth): truth[u] = [(start, end)] samples of every word"""
    rows, truth = [], []
    for u, (words, pauses) in enumerate(UTTERANCES):
        parts, at, spans = [np.zeros(LEAD_MS * SR // 1000)], LEAD_MS * SR // 1000, []
        for w, p in zip(words, pauses):
            x = burst(w)
            spans.append((at, at + len(x)))
            parts += [x, np.zeros(p * SR // 1000)]
            at += len(x) + p * SR // 1000
        x = np.concatenate(parts)
        rows.append((x + NOISE * np.random.RandomState(200 + u).randn(len(x))).astype(np.float32))
        truth.append(spans)
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    waves = np.zeros((len(rows), int(lens.max())), dtype=np.float32)
    for u, r in enumerate(rows):
        waves[u, :len(r)] = r
    return waves, lens, [list(w) for w, _ in UTTERANCES], truth


def boundary_errors(results, truth):
    """-> the largest |cut boundary - true boundary| in frames of 128 samples; asserts every word is cut, in order"""
    worst = 0.0
    for res, spans in zip(results, truth):
        assert res['dropped'] is None and len(res['cuts']) == len(spans), res
        starts = [a for _, a, _, _ in res['cuts']]
        assert starts == sorted(starts)
        for (_, a, z, _), (s, e) in zip(res['cuts'], spans):
            worst = max(worst, abs(a - s) / float(align.HOP), abs(z - e) / float(align.HOP))
    return worst


def cuts64():
    """the arbiter's cuts: path64 on float64 cepstra (align_model.melcep64) of the same utterances and templates"""
    waves, lens, transcripts, truth = utterances()
    pad = lambda c: np.concatenate([c, np.zeros((len(c), CEPW - c.shape[1]))], 1)          # noqa: E731
    templates = {w: pad(align_model.melcep64(x, [x.shape[1]])[0][1]) for w, x in template_store().items()}
    out = []
    for u, words in enumerate(transcripts):
        cep = pad(align_model.melcep64(waves[u:u + 1], lens[u:u + 1])[0][1])
        ref, offsets, lengths = align.reference_for(words, templates, cep)
        _, lo, hi = align.path64(cep, len(cep), ref, len(ref))
        out.append(dict(dropped=None, cuts=[(w,) + align.word_span(lo, hi, o, k, lens[u]) + (0.0,)
                                            for w, o, k in zip(words, offsets, lengths)]))
    return out, truth


# BOUNDARY.  The largest boundary error of ``cuts64`` on these utterances, in frames - the arbiter's own error: a frame spans
# 256 samples at hop 128, so a boundary is known to a frame or two at best - and the tolerance of every route that runs in
# fp32 (the models on the CPU, the kernels on the GPU): one frame more.  tests/test_dtwalign.py asserts that PATH64_WORST is
# what ``cuts64`` gives; both numbers are in profiles/dtw_align_fuzz.txt.
PATH64_WORST = 1.625          # frames: 208 samples (the end of 'alpha' in the second utterance, 4608 against 4400)
BOUNDARY_TOLERANCE = PATH64_WORST + 1.0          # 2.625 frames
