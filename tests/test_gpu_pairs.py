"""All-pairs DTW of the held-out evaluation on the GPU (-m gpu): kernels.dtw_pairs / ag_dtw_pairs bit for bit against
kernels.dtw_cost on gathered copies of the same pairs, in both forms and on both sides of the dispatch rule; the shared DTW
checkers of tests/align_model.py through an adaptor; evaluate.aligned_distance_matrix on the synthetic words; Evaluator(
aligned=True, crossed=True, draws=2) under the checks of tests/test_pairs.py; a training loop that evaluates with them.

Outputs are NaN-filled between guard floats; the inputs hold NaN past the counts and outside columns 1..12, so a read of
either shows.  No case feeds an index outside a bank: the clamp is stated by the CPU model alone."""
import pytest
import torch

from tests import test_evaluate as TE
from tests import test_pairs as TP
from tests.align_model import DTW_F, DTW_PAIRS, check_dtw_integer, check_dtw_properties, check_dtw_real, dtw_case
from tests.pairs_model import LISTS, WAVE_COUNTS, bank, check_pairs, check_words, pair_lists, paired_adaptor, run_guarded

WAVE, WG = 'dtw_pairs_wave_kernel', 'dtw_pairs_wg_kernel'


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    return K_


def _cuda(t):
    return t.cuda()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(K, form, ca, na, cb, nb, ia=None, ib=None):
    """dtw_pairs on the banks == dtw_cost on the gathered copies of the same pairs, bit for bit; the form; twice the same"""
    got = run_guarded(K.dtw_pairs, ca, na, cb, nb, ia, ib, on=_cuda)
    assert K.lib.ag_last_kernel().decode() == form
    I, J = (torch.from_numpy(v) for v in pair_lists(ca.size(0), cb.size(0), ia, ib))
    want = K.dtw_cost(ca[I].cuda(), na[I].cuda(), cb[J].cuda(), nb[J].cuda()).cpu()
    assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want)), (form, got, want)
    assert torch.equal(_bits(run_guarded(K.dtw_pairs, ca, na, cb, nb, ia, ib, on=_cuda)), _bits(got))
    return got


# ------------------------------------------------------------------------------------------------------------------
# bit identity with dtw_cost
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_wave_form_counts_cross_and_lists(K):
    """capacities 64 / 64: every pair of the counts 1, 2, 7, 33, 63, 64 (36 pairs), a 5 x 7 cross product (35 pairs: a
    partial last workgroup), index lists with repeats at P = 1, 4, 5"""
    ca, na = bank(WAVE_COUNTS, 64, False, 1)
    cb, nb = bank(WAVE_COUNTS[::-1], 64, False, 2)
    got = same_bits(K, WAVE, ca, na, cb, nb)
    assert got.numel() == 36
    check_pairs(K.dtw_pairs, ca, na, cb, nb, on=_cuda)
    c7, n7 = bank((64, 5, 33, 1, 63, 2, 7), 64, False, 3)
    same_bits(K, WAVE, ca[:5].contiguous(), na[:5].contiguous(), c7, n7)
    for P, (ia, ib) in LISTS.items():
        assert same_bits(K, WAVE, ca, na, cb, nb, ia, ib).numel() == P
    ci, ni = bank(WAVE_COUNTS, 64, True, 4)
    check_pairs(K.dtw_pairs, ci, ni, ci.flip(0).contiguous(), ni.flip(0).contiguous(), integer=True, on=_cuda)


@pytest.mark.gpu
def test_wave_form_long_columns_and_swapped_sides(K):
    """capacities 64 / 256 with counts (64, 256), (1, 256), (64, 1); capacities 132 / 64, where a is the longer side and the
    host exchanges the roles: the cross product still lands at [i * Nb + j]"""
    ca, na = bank((64, 1, 64), 64, False, 5)
    cb, nb = bank((256, 256, 1), 256, False, 6)
    same_bits(K, WAVE, ca, na, cb, nb, (0, 1, 2), (0, 1, 2))
    same_bits(K, WAVE, ca, na, cb, nb)
    same_bits(K, WAVE, cb, nb, ca, na, (0, 1, 2, 2), (0, 1, 2, 0))          # 256 / 64: swapped, with lists
    ca, na = bank((132, 1, 65), 132, False, 7)
    cb, nb = bank((64, 33, 1, 7), 64, False, 8)
    got = same_bits(K, WAVE, ca, na, cb, nb)
    assert got.numel() == 12
    check_pairs(K.dtw_pairs, ca, na, cb, nb, on=_cuda)


@pytest.mark.gpu
def test_dispatch_edge(K):
    """the rule is on the capacities: 64 | 65 on the shorter side, 256 | 257 on the longer"""
    for Fa, Fb, form in ((64, 64, WAVE), (65, 65, WG), (64, 65, WAVE), (65, 64, WAVE), (64, 256, WAVE), (64, 257, WG),
                         (257, 64, WG), (256, 64, WAVE)):
        ca, na = bank((min(Fa, 40), Fa, 1), Fa, False, 9)
        cb, nb = bank((Fb, 3), Fb, False, 10)
        same_bits(K, form, ca, na, cb, nb)


@pytest.mark.gpu
def test_workgroup_form(K):
    """capacities 132 / 132 with the pairs of align_model.DTW_PAIRS as lists, a 3 x 4 cross product, one pair of 1024 x 1024
    frames (integer inputs: exact against float64 as well)"""
    ca, na, cb, nb = dtw_case(DTW_PAIRS, DTW_F, DTW_F, False)
    idx = tuple(range(len(DTW_PAIRS)))
    same_bits(K, WG, ca, na, cb, nb, idx, idx)
    same_bits(K, WG, ca, na, cb, nb, idx[::-1], idx)
    same_bits(K, WG, ca[4:7].contiguous(), na[4:7].contiguous(), cb[6:10].contiguous(), nb[6:10].contiguous())
    ca, na, cb, nb = dtw_case(((1024, 1024),), 1024, 1024, True)
    same_bits(K, WG, ca, na, cb, nb)
    check_pairs(K.dtw_pairs, ca, na, cb, nb, integer=True, on=_cuda)


@pytest.mark.gpu
def test_shared_checkers_on_both_forms(K):
    """check_dtw_integer / check_dtw_real / check_dtw_properties with ia = ib = arange: at their own capacities (132, 1024)
    the workgroup form; with every pair that fits cut to capacity 64, the wave form"""
    fn = paired_adaptor(K.dtw_pairs)
    check_dtw_integer(fn, on=_cuda)
    check_dtw_real(fn, on=_cuda)
    check_dtw_properties(fn, on=_cuda)
    assert K.lib.ag_last_kernel().decode() == WG
    fn = paired_adaptor(K.dtw_pairs, F=64)
    check_dtw_integer(fn, on=_cuda, long=False)
    check_dtw_real(fn, on=_cuda)
    check_dtw_properties(fn, on=_cuda)
    assert fn.cut >= 3 * 5          # (1, 1), (1, 7), (7, 1), (2, 2), (63, 64) of DTW_PAIRS fit, in every pass


@pytest.mark.gpu
def test_dtw_pairs_bad_arguments(K):
    ca, na = bank((3, 2), 8, False, 1)
    with pytest.raises(RuntimeError):
        K.dtw_pairs(ca, na.cuda(), ca.cuda(), na.cuda())
    with pytest.raises(TypeError):
        K.dtw_pairs(ca.cuda().double(), na.cuda(), ca.cuda(), na.cuda())
    with pytest.raises(TypeError):
        K.dtw_pairs(ca.cuda(), na.cuda(), ca.cuda(), na.cuda(), ia=torch.zeros(2, dtype=torch.long, device='cuda'),
                    ib=torch.zeros(2, dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError):
        K.dtw_pairs(ca.cuda(), na.cuda(), ca.cuda(), na.cuda(), ia=torch.zeros(2, dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError):
        K.dtw_pairs(torch.zeros(1, 1025, 16, device='cuda'), None, torch.zeros(1, 4, 16, device='cuda'), None)


# ------------------------------------------------------------------------------------------------------------------
# higher levels
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_synthetic_words_gpu(K):
    from audiogan_amd.evaluate import aligned_distance, aligned_distance_matrix, crossed_scores
    check_words(aligned_distance_matrix, crossed_scores, on=_cuda)
    assert K.lib.ag_last_kernel().decode() == WAVE
    from tests.pairs_model import word_sets
    reals, rl, fakes, fl, _ = (t.cuda() for t in word_sets())
    assert torch.equal(aligned_distance_matrix(fakes, fl, reals, rl).diagonal(), aligned_distance(fakes, fl, reals, rl))


@pytest.mark.gpu
def test_crossed_run_gpu(K, tmp_path):
    import audiogan_amd as A
    K.lstm_persist_status(reset=True)
    s = TE._setup(A, torch.device('cuda'), 'toy_gpu', tmp_path, 8)
    TP.run_checks(s, tmp_path)
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0


@pytest.mark.gpu
def test_eager_loop_with_crossed_evaluator_changes_no_training_bit(K, tmp_path):
    """an eager TrainLoop of 2 passes at toy_gpu with Evaluator(aligned, crossed, draws=2) against one without an evaluator:
    every parameter and the CUDA generator state equal"""
    import audiogan_amd as A
    dev = torch.device('cuda')
    K.lstm_persist_status(reset=True)
    got = []
    for evaluating in (False, True):
        s = TE._setup(A, dev, 'toy_gpu', tmp_path, 8)
        torch.cuda.manual_seed(17)
        kw = dict(evaluator=TE._evaluator(s, aligned=True, crossed=True, draws=2), eval_every=1) if evaluating else {}
        lp = s.mk(fixed_critic_iter=2, gencatchup=1, stop='never', checkpoint_every=0, check=False, host=False, **kw)
        for _ in range(2):
            lp.outer()
        if evaluating:
            assert len(lp.eval_log) == 2
            assert all(r['nn_db'] > 0 and r['div_db'] >= 0 and 0 <= r['word_hit'] <= 1 for r in lp.eval_log)
        got.append(([p.detach().clone() for m in s.mods for p in m.parameters()], torch.cuda.get_rng_state()))
    for a, b in zip(got[0][0], got[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(got[0][1], got[1][1])
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0
