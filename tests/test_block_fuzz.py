"""-m gpu: the autograd blocks against float64 (tests/block_cases.py) - every ``torch.autograd.Function`` between the kernels
and the networks called directly with a hand-built GTrunk / DConvStack / DHead / LSTM layer, at the smallest shapes that
select each branch, under every gradient route: fresh gradient tensors, direct accumulation into ``.grad`` from a zero and
from a random start, inside ``common.network_backward()`` from both starts, applied twice inside one scope (the
``finish_pending`` path), under ``common.frozen`` wholly, and partly with the freeze active while the forward runs and while
the backward of an unfrozen forward runs (the stopper-only order) onto preset ``.grad``, with an input that takes no
gradient, and with a ``.grad`` that ``grad_target`` must refuse.

Every output, input gradient and parameter gradient is held to float64 under the bound rule of DESIGN.md section 2 (the
floor is the CPU kernel model's error on the same case and route, computed here before the GPU runs; 16 x floor, never
above 1e-4 of the scale); direct accumulation and deferral must not change a bit against the fresh route; a frozen block
must leave every ``.grad`` bit-unchanged; every case runs twice for identical bits; the sticky status word of the
persistent launches is read after every run and a non-zero word fails the test at once.  Each test asserts, by counting
the kernel wrappers a case went through and with the library's own ``*_ok`` predicates, that the case took the branch it
stands for, and begins with the family's coverage assertion.  Each prints the largest error / floor per block and output
(``pytest -s``; profiles/block_fuzz.txt).  tests/test_block_fuzz_host.py shows on the CPU model that the sweep rejects
subtly wrong blocks."""
import contextlib
import time

import pytest
import torch

from tests import block_cases as BC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def floors():
    """the CPU kernel model's error on every case and route, and on the weight-cache cases (computed before any GPU run;
    the model is installed for this block only)"""
    out, cache = {}, {}
    with pytest.MonkeyPatch.context() as mp:
        BC.install_model(mp)
        for name, fam in BC.FAMILIES.items():
            out[name] = BC.floors(fam)
            for i in BC.CACHE_CASES.get(name, ()):
                cache[(name, i)] = BC.cache_floors(fam, fam.cases()[i])
    return out, cache


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    assert K_.gemm.__module__ == 'audiogan_amd.kernels', 'real kernels must be in place'
    assert K_.LEAKY_SLOPE == BC.SLOPE
    return K_


def _dev():
    return torch.device('cuda', torch.cuda.current_device())


def _status(K):
    def after(case, route):
        st = K.lstm_persist_status()
        assert st == 0, ('a persistent launch gave up', case['id'], route, K.persist_error_text(st))
    return after


def _report(name, worst, t0):
    for form in sorted(worst):
        print('block fuzz | %-22s | %s' % (form, '  '.join('%s %.2f' % kv if kv[1] >= 0.1 else '%s %.4f' % kv for kv in sorted(worst[form].items()))))
    print('block fuzz | %-22s | wall time %.1f s' % (name, time.time() - t0))


def _run(K, floors, name, names, expect_case):
    """the family's sweep with the wrappers `names` counted per case; expect_case(case, counts) asserts the branch"""
    fam = BC.FAMILIES[name]
    BC.assert_coverage(name)
    K.lstm_persist_status(reset=True)
    t0 = time.time()

    @contextlib.contextmanager
    def expect(case):
        with BC.counting(K, names) as n:
            yield
        expect_case(case, n)
    with K.precision('f32'):
        worst = BC.sweep(fam, _dev(), floors[0][name], after=_status(K), expect=expect)
        for i in BC.CACHE_CASES.get(name, ()):
            case = fam.cases()[i]
            BC.merge_worst(worst, '%s weight cache (%s)' % (name, case['mode'] if 'mode' in case else 'f32'),
                           BC.check_cache(fam, case, _dev(), floors[1][(name, i)]))
            if name != 'lstm':          # (LSTMSeqFn keeps no materialised weights: it has no such assertion)
                BC.check_changed_between(fam, case, _dev())
    _status(K)(dict(id=name), 'end')
    _report(name, worst, t0)


def test_gtrunk_vs_float64(K, floors):
    def expect(c, n):
        o1 = K.conv_o1_ok('conv', 1, c['fk'], 1, (c['fk'] - 1) // 2)
        assert o1 == (('final', 'o1') in BC.FAMILIES['gtrunk'].classes(c))
        assert (n['conv_o1_fwd'] > 0) == o1 and (n['conv_o1_bwd_data'] > 0) == o1 and (n['conv_o1_wgrad'] > 0) == o1, (c, dict(n))
        assert n['conv_engine'] > 0 and n[('conv_engine', K.ACT_LEAKY_GATE)] > 0
    _run(K, floors, 'gtrunk', ('conv_o1_fwd', 'conv_o1_bwd_data', 'conv_o1_wgrad', 'conv_engine', 'leaky_bwd'), expect)


def test_dconvstack_vs_float64(K, floors):
    def expect(c, n):
        pat = c['pat']
        top = max(i for i, on in enumerate(pat) if on)
        gated = sum(1 for i in range(1, top + 1) if not pat[i - 1])
        assert (n['axpby'] > 0) == (sum(pat) > 1), (c, dict(n))
        assert (n[('conv_engine', K.ACT_LEAKY_GATE)] > 0) == (gated > 0), (c, dict(n))
        assert n['conv_o1_fwd'] == 0
    _run(K, floors, 'dconv', ('axpby', 'conv_engine', 'leaky_bwd', 'channel_sum', 'conv_o1_fwd'), expect)


def test_dhead_vs_float64(K, floors):
    def expect(c, n):
        rd = c['n_out'] == 1
        assert rd == BC.rowdot_ok_sizes(c['n_out'])
        assert (n['rowdot_fwd'] > 0) == rd and (n['rowdot_bwd'] > 0) == rd, (c, dict(n))
        assert n['bct_to_tbc'] > 0 and n['tbc_to_bct'] > 0
        # bf16 rows reach ag_gemm_h at state 64 and only there: at 48 every product is widened (ops._gh's fall-back)
        assert (n['gemm_h'] > 0) == (c['mode'] == 'gate'), (c, dict(n))
        assert (n['to_bf16'] > 0) == (c['mode'] in ('gate', 'widen')), (c, dict(n))
        if c['mode'] in ('f32', 'add'):
            assert (n[('gemm', K.ACT_LEAKY_GATE)] > 0) == (c['n_res'] > 0 or not rd), (c, dict(n))
        if c['mode'] == 'add' and c['n_res'] > 1:
            assert n['act_bwd'] > 0, (c, dict(n))          # the skip stays an fp32 add, the gate a pass of its own
        if c['mode'] == 'f32':
            assert n['act_bwd'] == 0, (c, dict(n))
    _run(K, floors, 'dhead', ('rowdot_fwd', 'rowdot_bwd', 'gemm', 'gemm_h', 'act_bwd', 'bct_to_tbc', 'tbc_to_bct', 'to_bf16'), expect)


def test_lstmseq_vs_float64(K, floors):
    dev = _dev()
    met = set()
    sums = []
    real_bwd = K.lstm_seq_bwd

    def logged(*a, **k):
        r = real_bwd(*a, **k)
        sums.append((bool(r), k.get('dgsum') is not None))
        return r

    def expect(c, n):
        B, H, nd = c['B'], c['H'], c['ndir']
        fused = K.lstm_step_ok(B, H)
        persist = fused and K.lstm_persist_ok(B, H, nd, dev) and K.lstm_persist_bwd_ok(B, H, nd, dev)
        assert fused == BC.lstm_step_ok(B, H)
        assert persist == (c['cls'] == 'persist'), ('this device does not run the case as its class says', c)
        if c['cls'] == 'fused':
            assert not K.lstm_persist_ok(B, H, nd, dev) and not K.lstm_persist_bwd_ok(B, H, nd, dev), c
        assert (n['_lstm_seq_fwd_persist_call'] > 0) == persist and (n['_lstm_seq_bwd_persist_call'] > 0) == persist, (c, dict(n))
        assert (n['lstm_seq_fwd'] > 0) == fused and (n['lstm_cell_fwd'] > 0) == (not fused), (c, dict(n))
        assert (n['lstm_cell_bwd'] > 0) == (not BC.lstm_bwd_seq(B, H)), (c, dict(n))
        if c['mode'] == 'x16':          # bf16-stored x: the input projections on ag_gemm_h where the input width allows
            assert n['gemm_h'] > 0 or c['Fx'] % 64 != 0, (c, dict(n))
        else:
            assert n['gemm_h'] == 0
        met.add(c['cls'])
    K.lstm_seq_bwd = logged
    try:
        _run(K, floors, 'lstm', ('lstm_seq_fwd', '_lstm_seq_fwd_persist_call', '_lstm_seq_bwd_persist_call', 'lstm_cell_fwd',
                                 'lstm_cell_bwd', 'gemm_h'), expect)
    finally:
        K.lstm_seq_bwd = real_bwd
    assert met == {'persist', 'fused', 'loop', 'loop_fwd', 'wide'}
    # the time sum of dgates: made by the launch itself (persistent backward) and left to a pass of the Function's own
    assert (True, True) in sums and (False, True) in sums and (False, False) in sums, set(sums)


def test_small_functions_vs_float64(K, floors):
    names = ('build_zc', 'critic_batch', 'bce_logits_fwd_strided', 'bce_logits_bwd_strided', 'time_moments_fwd',
             'time_moments_bwd', 'bce_logits_fwd', 'bce_logits_bwd')
    # each case runs its one route twice: the launches of its Function, forward and backward, twice each and no other
    want = dict(buildzc=('build_zc',), critic_input=('critic_batch',), bce=('bce_logits_fwd_strided', 'bce_logits_bwd_strided'),
                moments=('time_moments_fwd', 'time_moments_bwd'), per_sample=('bce_logits_fwd', 'bce_logits_bwd'))
    seen = []
    real = {k: getattr(K, k) for k in ('bce_logits_fwd_strided', 'bce_logits_bwd_strided')}

    def expect(c, n):
        got = {k: n[k] for k in names if n[k]}
        assert got == {k: 2 for k in want[c['op']]}, (c, got)
        if c['op'] == 'bce':
            # the logits reach both launches as the view they are (a transposed view: not contiguous, no copy was made)
            assert len(seen) == 4 and all(cont == (c['view'] != 't') for cont in seen), (c, seen)
        del seen[:]
    for k, f in real.items():
        setattr(K, k, lambda x, *a, _f=f, **kw: (seen.append(x.is_contiguous()), _f(x, *a, **kw))[1])
    try:
        _run(K, floors, 'small', names, expect)
    finally:
        for k, f in real.items():
            setattr(K, k, f)
    BC.bce_backward_without_gradient()


def test_convchain_linear_vs_float64(K, floors):
    def expect(c, n):
        assert n['prep_conv_weight'] > 0 and n['conv_engine'] > 0 and n['gemm'] > 0 and n['col_sum'] > 0, (c, dict(n))
    _run(K, floors, 'chain', ('prep_conv_weight', 'conv_engine', 'conv_wgrad', 'gemm', 'col_sum'), expect)
