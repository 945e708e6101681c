"""All-pairs DTW of the held-out evaluation on the CPU: the model of kernels.dtw_pairs (tests/pairs_model.py) against float64
and the mutants its checker must reject, ag_dtw_pairs' refusals (host code, no GPU), evaluate.crossed_scores and
evaluate.aligned_distance_matrix, and Evaluator(aligned=True, crossed=True, draws=k) on the kernel models.  The GPU half is
tests/test_gpu_pairs.py, which runs ``run_checks`` of this file on the HIP kernels.

Bounds: tests/align_model.py (integer inputs bit for bit; real inputs within dtw_real_bound of float64, summed where a
number is a mean of many pairs)."""
import collections
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import align_model, eval_model, kernel_model, pairs_model
from tests import test_evaluate as TE
from tests.align_model import dtw64, dtw_real_bound
from tests.pairs_model import LISTS, MUTANTS, check_pairs, check_words, rect_case

MCD_DB = 10.0 / math.log(10.0) * math.sqrt(2.0)
NEW_KEYS = ('nn_db', 'cover_db', 'word_hit', 'word_hit/chance', 'div_db', 'real_div_db')


def _models(monkeypatch):
    kernel_model.install(monkeypatch)
    eval_model.install(monkeypatch)
    align_model.install(monkeypatch)
    pairs_model.install(monkeypatch)


# ------------------------------------------------------------------------------------------------------------------
# the model under its checker
# ------------------------------------------------------------------------------------------------------------------
def test_pairs_model_against_float64():
    for integer in (True, False):
        ca, na, cb, nb = rect_case(integer)
        check_pairs(pairs_model.dtw_pairs, ca, na, cb, nb, integer=integer)
        for P, (ia, ib) in LISTS.items():
            assert len(ia) == len(ib) == P
            check_pairs(pairs_model.dtw_pairs, ca[:6], na[:6], cb[:6], nb[:6], ia, ib, integer=integer)


def test_pairs_model_layout_and_clamp():
    """out[i * Nb + j] is pair (i, j); an index outside a bank is the nearest one inside it"""
    ca, na, cb, nb = rect_case(False)
    cross = pairs_model.dtw_pairs(ca, na, cb, nb)
    assert tuple(cross.shape) == (5, 7)
    one = align_model.dtw_cost(ca[3:4], na[3:4], cb[5:6], nb[5:6])
    assert torch.equal(cross[3, 5:6], one)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)          # noqa: E731
    got = pairs_model.dtw_pairs(ca, na, cb, nb, ia=i32([-4, 5, 99, 2]), ib=i32([0, -1, 7, 6]))
    assert torch.equal(got, torch.stack([cross[0, 0], cross[4, 0], cross[4, 6], cross[2, 6]]))
    # counts of None are the capacities
    fa, fb = ca[1:2], cb[:1]
    assert torch.equal(pairs_model.dtw_pairs(fa, None, fb, None), cross[1:2, :1]) and int(na[1]) == 20 and int(nb[0]) == 12


@pytest.mark.parametrize('mutant', MUTANTS)
def test_pairs_checker_rejects_mutants(mutant):
    """the output transposed, nf_b taken at ia, indices off by one, counts clamped to the other side's capacity: the
    rectangular cross product fails in the integer pass and in the real pass"""
    fn = lambda *a, **k: pairs_model.dtw_pairs(*a, mutate=mutant, **k)          # noqa: E731
    for integer in (True, False):
        ca, na, cb, nb = rect_case(integer)
        with pytest.raises(AssertionError):
            check_pairs(fn, ca, na, cb, nb, integer=integer)


_HOST = ctypes.create_string_buffer(64 + 16)
PTR = (ctypes.addressof(_HOST) + 15) & ~15


def test_launcher_refuses_before_any_hip_call():
    """every refusal of ag_dtw_pairs: AG_ERR_ARG from host code, with no device in sight (the pointers are host memory: a
    launch would not survive them)"""
    import audiogan_amd.kernels as K
    from audiogan_amd import _lib
    p = ctypes.c_void_p(PTR)
    ok = dict(ca=p, na=p, Na=3, Fa=8, cb=p, nb=p, Nb=4, Fb=8, ia=p, ib=p, out=p, P=5)

    def call(**bad):
        a = dict(ok, **bad)
        return K.lib.ag_dtw_pairs(a['ca'], a['na'], a['Na'], a['Fa'], a['cb'], a['nb'], a['Nb'], a['Fb'], a['ia'], a['ib'],
                                  a['out'], a['P'], None)
    for bad in (dict(Fa=0), dict(Fb=0), dict(Fa=1025), dict(Fb=1025)):
        assert call(**bad) == _lib.AG_ERR_ARG, bad
        assert b'1024' in K.lib.ag_last_error()
    for bad in (dict(ca=None), dict(cb=None), dict(out=None), dict(ia=None), dict(ib=None), dict(P=0), dict(P=-1),
                dict(P=(1 << 24) + 1), dict(ia=None, ib=None, P=11), dict(ia=None, ib=None, P=13), dict(Na=0), dict(Nb=0),
                dict(Na=65536), dict(Nb=65536), dict(ia=None, ib=None, Na=65535, Nb=65535, P=1)):
        assert call(**bad) == _lib.AG_ERR_ARG, bad
        assert K.lib.ag_last_error().startswith(b'ag_dtw_pairs')
    assert K.lib.ag_abi_version() == 13


# ------------------------------------------------------------------------------------------------------------------
# crossed_scores, aligned_distance_matrix
# ------------------------------------------------------------------------------------------------------------------
def test_crossed_scores_on_hand_made_matrices():
    from audiogan_amd.evaluate import crossed_scores
    M = torch.tensor([[1.0, 2.0, 3.0],
                      [4.0, 0.5, 0.5],          # a tie between the own word's column (2) and another: a hit
                      [2.0, 7.0, 6.0],          # the nearest clip is another word's: a miss
                      [5.0, 5.0, 0.25]])
    same = torch.tensor([[1, 0, 0], [0, 0, 1], [0, 0, 1], [0, 1, 0]], dtype=torch.bool)
    s = crossed_scores(M, same)
    assert s == dict(nn_db=(1.0 + 0.5 + 2.0 + 0.25) / 4, cover_db=(1.0 + 0.5 + 0.25) / 3, word_hit=0.5, chance=1.0 / 3)
    # a repeated word: fakes 0 and 1 say the word of real clips 0 and 2; fake 1's nearest is the SECOND clip of its word
    same = torch.tensor([[1, 0, 1], [1, 0, 1], [0, 1, 0], [0, 0, 0]], dtype=torch.bool)
    s = crossed_scores(M.numpy(), same.numpy())
    assert abs(s['chance'] - (2 + 2 + 1 + 0) / 3.0 / 4) < 1e-15 and s['word_hit'] == 0.5
    assert crossed_scores(M[:, :1], same[:, :1])['cover_db'] == 1.0


def test_option_refusals(monkeypatch, tmp_path):
    _models(monkeypatch)
    import audiogan_amd as A
    s = TE._setup(A, torch.device('cpu'), 'toy', tmp_path, 4)
    for kw in (dict(crossed=True), dict(draws=2), dict(crossed=True, draws=3)):
        with pytest.raises(ValueError, match='aligned'):
            TE._evaluator(s, **kw)
    with pytest.raises(ValueError):
        TE._evaluator(s, aligned=True, draws=0)


def test_distance_matrix_matches_the_paired_distance(monkeypatch):
    _models(monkeypatch)
    from audiogan_amd.evaluate import aligned_distance, aligned_distance_matrix
    g = torch.Generator().manual_seed(4)
    a, b = torch.randn(3, 1100, generator=g), torch.randn(2, 700, generator=g)
    la, lb = torch.tensor([1100, 640, 90]), torch.tensor([700, 300])
    M = aligned_distance_matrix(a, la, b, lb)
    assert M.dtype == torch.float64 and tuple(M.shape) == (3, 2)
    for j in range(2):
        assert torch.equal(M[:, j], aligned_distance(a, la, b[j:j + 1].repeat(3, 1), lb[j:j + 1].repeat(3)))
    with pytest.raises(ValueError):
        aligned_distance_matrix(a, la, torch.zeros(1, 131329), None)


def test_synthetic_words_on_the_models(monkeypatch):
    _models(monkeypatch)
    from audiogan_amd.evaluate import aligned_distance_matrix, crossed_scores
    check_words(aligned_distance_matrix, crossed_scores)


# ------------------------------------------------------------------------------------------------------------------
# the evaluator
# ------------------------------------------------------------------------------------------------------------------
def reworded(heldout, words):
    """the held-out minibatches with the words replaced: ``words`` [batches][B] small integers, one character each"""
    out = []
    for mb, ws in zip(heldout, words):
        mb = list(mb)
        cseq, clen = np.zeros_like(np.asarray(mb[5])), np.ones_like(np.asarray(mb[6]))
        cseq[:, 0] = 97 + np.asarray(ws)
        mb[5], mb[6] = cseq, clen
        out.append(mb)
    return out


def words_for(B, repeats=True):
    """two minibatches of B words: with repeats inside a minibatch and across the two, or all different"""
    if not repeats:
        return [list(range(B)), list(range(B, 2 * B))]
    first = list(range(B))
    first[2] = 0                                   # clips 0 and 2 share a word
    second = list(range(B, 2 * B))
    second[1], second[-1] = 1, second[-2]          # one word of the first minibatch again, and a repeat of its own
    return [first, second]


def _gather64(cep_a, nf_a, I, cep_b, nf_b, J):
    """float64 totals and bounds of the pairs (I, J)"""
    n, m = nf_a[I], nf_b[J]
    D = dtw64(cep_a[I], n, cep_b[J], m)
    return D, np.array([dtw_real_bound(a, b, d) for a, b, d in zip(n, m, D)]), (n + m).astype(np.float64)


def restate_new_keys(res, parts, ev, words):
    """every new number from the returned parts in float64, within the real-pass bound summed over what the number averages"""
    B, k = ev.B, ev.draws
    nn = cover = hits = chance = div = 0.0
    tol_nn = tol_cover = tol_div = 0.0
    for p, ws in zip(parts, words):
        same = np.array([[a == b for b in ws] for a in ws])
        assert np.array_equal(p['same'].cpu().numpy(), same) and tuple(p['cross'].shape) == (B, B)
        assert p['cross'].dtype == torch.float32
        nf, rnf = p['nf'].cpu().numpy(), p['real_nf'].cpu().numpy()
        I, J = pairs_model.pair_lists(B, B)
        D, bound, w = _gather64(p['cep'].cpu().numpy(), nf, I, p['real_cep'].cpu().numpy(), rnf, J)
        got = p['cross'].cpu().double().numpy().reshape(-1)
        assert (np.abs(got - D) <= bound).all(), (got, D)
        M64, T = (MCD_DB * D / w).reshape(B, B), (MCD_DB * bound / w).reshape(B, B)
        nn, tol_nn = nn + M64.min(1).sum(), tol_nn + T.max(1).sum()          # |min got - min want| <= the row's largest bound
        cover, tol_cover = cover + M64.min(0).sum(), tol_cover + T.max(0).sum()
        M = (MCD_DB * got / w).reshape(B, B)          # the hit rule on the totals that were returned: ==, no argmin
        hits += sum(bool((same[i] & (M[i] == M[i].min())).any()) for i in range(B))
        chance += (same.sum(1) / float(B)).sum()
        # the draws
        bank, bnf = p['bank_cep'].cpu().numpy(), p['bank_nf'].cpu().numpy()
        ia, ib = p['pair_ia'].cpu().numpy(), p['pair_ib'].cpu().numpy()
        assert bank.shape[0] == k * B == bnf.shape[0] and np.array_equal(bnf[:B], nf)
        assert np.array_equal(bank[:B, :p['cep'].shape[1]][:, :nf.min()], p['cep'].cpu().numpy()[:, :nf.min()])
        want_pairs = [(a * B + b, c * B + b) for a in range(k) for c in range(a + 1, k) for b in range(B)]
        assert list(zip(ia.tolist(), ib.tolist())) == want_pairs
        D, bound, w = _gather64(bank, bnf, ia, bank, bnf, ib)
        got = p['pair_dtw'].cpu().double().numpy()
        assert (np.abs(got - D) <= bound).all(), (got, D)
        div, tol_div = div + (MCD_DB * D / w).sum(), tol_div + (MCD_DB * bound / w).sum()
    clips, npairs = ev.clips, ev.clips * k * (k - 1) // 2
    print('nn_db %r want %r; cover_db %r want %r; word_hit %r want %r; chance %r; div_db %r want %r' %
          (res['nn_db'], nn / clips, res['cover_db'], cover / clips, res['word_hit'], hits / clips, res['word_hit/chance'],
           res['div_db'], div / npairs))
    assert abs(res['nn_db'] - nn / clips) <= tol_nn / clips + 1e-12 * nn
    assert abs(res['cover_db'] - cover / clips) <= tol_cover / clips + 1e-12 * cover
    assert res['word_hit'] == hits / clips and abs(res['word_hit/chance'] - chance / clips) <= 1e-12
    assert abs(res['div_db'] - div / npairs) <= tol_div / npairs + 1e-12 * div
    # real_div_db: all pairs i < j of the held-out real clips with the same word
    flat = [w_ for ws in words for w_ in ws]
    ij = [(i, j) for i in range(len(flat)) for j in range(i + 1, len(flat)) if flat[i] == flat[j]]
    if not ij:
        assert res['real_div_db'] is None
        return
    cep = np.concatenate([p['real_cep'].cpu().numpy() for p in parts])
    rnf = np.concatenate([p['real_nf'].cpu().numpy() for p in parts])
    I, J = (np.array(c) for c in zip(*ij))
    D, bound, w = _gather64(cep, rnf, I, cep, rnf, J)
    want, tol = (MCD_DB * D / w).mean(), (MCD_DB * bound / w).mean()
    print('real_div_db %r want %r over %d pairs' % (res['real_div_db'], want, len(ij)))
    assert isinstance(res['real_div_db'], float) and abs(res['real_div_db'] - want) <= tol + 1e-12 * want


def run_checks(s, tmp_path, draws=2):
    """Evaluator(aligned, crossed, draws) on the setup ``s`` (tests.test_evaluate._setup): key set, float64 restatement,
    shared keys and first draws bit for bit those of an evaluator without the options, no generator and no .grad moved, a
    second pass equal, the dict through on_eval and the JSON line unchanged"""
    words = words_for(s.B)
    s.heldout = reworded(s.heldout, words)
    seen = []
    path = os.path.join(tmp_path, 'pairs.jsonl')
    state = (torch.random.get_rng_state(), np.random.get_state(),
             torch.cuda.get_rng_state() if s.dev.type == 'cuda' else None)
    ev = TE._evaluator(s, on_eval=seen.append, path=path, aligned=True, crossed=True, draws=draws)
    assert all(len(mb['more']) == draws - 1 and mb['same'].dtype == torch.bool for mb in ev.set)
    res, parts = ev.run(gen_iter=3, dis_iter=5, parts=True)
    assert set(res) == set(TE.FLOATS) | set(TE.INTS) | {'mcd_db'} | set(NEW_KEYS)
    assert all(isinstance(res[k], float) and math.isfinite(res[k]) for k in NEW_KEYS)
    assert res['nn_db'] > 0 and res['cover_db'] > 0 and res['div_db'] >= 0 and res['real_div_db'] > 0
    assert 0.0 <= res['word_hit'] <= 1.0 and res['word_hit/chance'] > 1.0 / s.B
    restate_new_keys(res, parts, ev, words)
    res2 = ev.run(gen_iter=3, dis_iter=5)
    assert res2 == res and seen == [res, res2]
    with open(path) as f:
        assert [json.loads(ln) for ln in f] == [dict(kind='E', **res), dict(kind='E', **res2)]
    assert torch.equal(torch.random.get_rng_state(), state[0])
    st = np.random.get_state()
    assert st[0] == state[1][0] and np.array_equal(st[1], state[1][1]) and st[2:] == state[1][2:]
    if state[2] is not None:
        assert torch.equal(torch.cuda.get_rng_state(), state[2])
    assert all(p.grad is None for m in s.mods for p in m.parameters())
    # without the new options: today's keys, every shared number and every first draw with the same bits
    base = TE._evaluator(s, aligned=True)
    assert all(torch.equal(a['z'], b['z']) and torch.equal(a['u'], b['u']) for a, b in zip(ev.set, base.set))
    assert not any('more' in mb or 'same' in mb for mb in base.set)
    old = base.run(gen_iter=3, dis_iter=5)
    assert set(old) == set(TE.FLOATS) | set(TE.INTS) | {'mcd_db'} and all(old[k] == res[k] for k in old)
    plain = TE._evaluator(s).run(gen_iter=3, dis_iter=5)
    assert set(plain) == set(TE.FLOATS) | set(TE.INTS) and all(plain[k] == res[k] for k in plain)
    return res


def test_crossed_run_on_toy_networks(monkeypatch, tmp_path):
    _models(monkeypatch)
    import audiogan_amd as A
    s = TE._setup(A, torch.device('cpu'), 'toy', tmp_path, 4)
    run_checks(s, tmp_path)


def test_three_draws_on_toy_networks(monkeypatch, tmp_path):
    """draws=3: three draw pairs per clip; crossed off, so only the two diversity keys are added"""
    _models(monkeypatch)
    import audiogan_amd as A
    s = TE._setup(A, torch.device('cpu'), 'toy', tmp_path, 4)
    ev = TE._evaluator(s, aligned=True, draws=3)
    res, parts = ev.run(parts=True)
    assert set(res) == set(TE.FLOATS) | set(TE.INTS) | {'mcd_db', 'div_db', 'real_div_db'}
    assert all(tuple(p['pair_dtw'].shape) == (3 * 4,) and 'cross' not in p for p in parts)
    two = TE._evaluator(s, aligned=True, draws=2)
    assert torch.equal(ev.set[0]['more'][0][0], two.set[0]['more'][0][0]) and len(ev.set[1]['more']) == 2
    assert all(torch.equal(a['z'], b['z']) and torch.equal(a['u'], b['u']) for a, b in zip(ev.set, two.set))


def test_real_diversity_is_none_without_a_repeated_word(monkeypatch, tmp_path):
    _models(monkeypatch)
    import audiogan_amd as A
    s = TE._setup(A, torch.device('cpu'), 'toy', tmp_path, 4)
    held = s.heldout
    s.heldout = reworded(held, words_for(4, repeats=False))
    ev = TE._evaluator(s, aligned=True, crossed=True, draws=2)
    res = ev.run()
    assert ev.real_div_db is None and res['real_div_db'] is None and res['word_hit/chance'] == 0.25
    assert isinstance(res['div_db'], float)
    s.heldout = reworded(held, words_for(4))
    ev = TE._evaluator(s, aligned=True, draws=2)
    assert isinstance(ev.real_div_db, float) and ev.real_div_db > 0 and ev.run()['real_div_db'] == ev.real_div_db


def test_call_counts(monkeypatch, tmp_path):
    """with ``aligned`` alone no dtw_pairs call; with the options: per held-out minibatch one dtw_pairs for the cross product
    and one for the draws, one melcep_frames per extra draw, no further critic or spectrum call; one dtw_pairs at
    construction for real_div_db"""
    _models(monkeypatch)
    import audiogan_amd as A
    import audiogan_amd.kernels as K
    calls = []

    def wrap(name, fn):
        def rec(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return rec
    for n in pairs_model.ALL + align_model.ALL + eval_model.ALL:
        monkeypatch.setattr(K, n, wrap(n, getattr(K, n)))
    s = TE._setup(A, torch.device('cpu'), 'toy', tmp_path, 4)
    s.heldout = reworded(s.heldout, words_for(4))
    TE._evaluator(s).run()
    n = collections.Counter(calls)
    assert n['melcep_frames'] == n['dtw_cost'] == n['dtw_pairs'] == 0 and n['ltas_power'] == 2 + 2 and n['score_accum'] == 2 * 2
    calls[:] = []
    TE._evaluator(s, aligned=True).run()
    n = collections.Counter(calls)
    assert n['dtw_pairs'] == 0
    assert n['melcep_frames'] == 2 + 2 and n['dtw_cost'] == 2 and n['ltas_power'] == 2 + 2 and n['score_accum'] == 2 * 2
    calls[:] = []
    ev = TE._evaluator(s, aligned=True, crossed=True, draws=3)
    n = collections.Counter(calls)
    assert n['dtw_pairs'] == 1 and n['melcep_frames'] == 2 and n['ltas_power'] == 2 and n['dtw_cost'] == 0
    calls[:] = []
    ev.run()
    n = collections.Counter(calls)
    assert n['dtw_pairs'] == 2 + 2 and n['melcep_frames'] == 2 * 3 and n['dtw_cost'] == 2
    assert n['ltas_power'] == 2 and n['score_accum'] == 2 * 2
    calls[:] = []
    TE._evaluator(s, aligned=True, crossed=True).run()
    n = collections.Counter(calls)
    assert n['dtw_pairs'] == 2 and n['melcep_frames'] == 2 + 2 and n['dtw_cost'] == 2
