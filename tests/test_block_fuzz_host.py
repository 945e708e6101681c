"""The autograd block fuzz (tests/block_cases.py) against the CPU model of the kernels: the tables, float64 references,
runner and checkers that tests/test_block_fuzz.py turns on the HIP kernels are shown here, without a GPU, to (a) meet
their own coverage assertions, (b) accept the Functions as they are on every case under every gradient route, with the
route bit equalities and the weight-cache checks, and (c) REJECT Functions that are subtly wrong.  Each mutant patches a
Function's helper or a kernel-model call INSIDE the test only - the product is not touched - and is a mistake the host
logic of a block can make: a dropped accumulation, a mask taken from the neighbouring layer, a lost residual gradient, a
missing identity, a time shift, a missing direction, a .grad overwritten, a stale weight cache, a scratch buffer reused
before its reader ran, a freeze overlooked at backward or at forward time.  Each mutant reports that the call it patches
was reached, so a layout change that turns one into a no-op fails with that message."""
import re

import pytest
import torch

from tests import block_cases as BC


@pytest.fixture(scope='module')
def floors():
    """{family: {(case id, route): errors of the unmutated model}}, computed once"""
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        BC.install_model(mp)
        for name, fam in BC.FAMILIES.items():
            out[name] = BC.floors(fam)
    return out


@pytest.fixture
def model(monkeypatch):
    return BC.install_model(monkeypatch)


@pytest.mark.parametrize('name', list(BC.FAMILIES))
def test_sweep_accepts_the_functions_on_the_model(model, floors, name):
    fam = BC.FAMILIES[name]
    BC.assert_coverage(name)
    worst = BC.sweep(fam, 'cpu', floors[name])
    assert worst and all(v == v for r in worst.values() for v in r.values())


@pytest.mark.parametrize('name', list(BC.FAMILIES))
def test_every_bound_is_finite_and_below_the_ceiling(floors, name):
    hi = 0.0
    for key, fl in floors[name].items():
        for out, (f, scale) in fl.items():
            assert f == f and 0 <= f < float('inf') and 0 < scale < float('inf'), (key, out, f, scale)
            assert 0 < BC.bound(BC.MARGIN_MAX, f) <= BC.CEIL
            hi = max(hi, f)
    # the fp32 model against float64 on these small tensors: an order below the 1e-4 ceiling, which therefore cuts into
    # the margin only on the few tensors whose floor is above 1e-4 / 16
    assert hi < BC.CEIL / 10, (name, hi)


def test_tables_are_seeded_and_a_dropped_class_is_noticed():
    for name, fam in BC.FAMILIES.items():
        assert fam.cases() == fam.cases()
        assert len(set(c['id'] for c in fam.cases())) == len(fam.cases())
        BC.assert_coverage(name)
    drop = dict(gtrunk=lambda c: c['place'] != 'view_off', dconv=lambda c: c['pat'] != (0, 1, 0, 0) and c['pat'] != (0, 0, 1, 0),
                dhead=lambda c: c['n_res'] != 0, lstm=lambda c: c['cls'] != 'wide', small=lambda c: c['op'] != 'moments',
                chain=lambda c: c['kind'] != 'convT')
    for name, keep in drop.items():
        with pytest.raises(AssertionError, match='no longer holds'):
            BC.assert_coverage(name, [c for c in BC.FAMILIES[name].cases() if keep(c)])
    a, b = BC.values(BC.FAMILIES['dhead'], BC.FAMILIES['dhead'].cases()[0]), BC.values(BC.FAMILIES['dhead'], BC.FAMILIES['dhead'].cases()[1])
    assert not torch.equal(a['xs'][0].flatten()[:4], b['xs'][0].flatten()[:4])


def test_restated_predicates_are_the_librarys():
    """the branch predicates block_cases restates from sizes alone, against audiogan_amd.kernels' own (pure host code)"""
    import audiogan_amd.kernels as K
    for k in range(1, 14):
        for cout in (1, 2):
            for stride in (1, 2):
                for pad in range(0, 7):
                    assert BC.conv_o1_ok('conv', cout, k, stride, pad) == K.conv_o1_ok('conv', cout, k, stride, pad)
    assert not K.conv_o1_ok('convT', 1, 5, 1, 2) and not BC.conv_o1_ok('convT', 1, 5, 1, 2)
    for B in (1, 4, 256, 257):
        for H in (4, 8, 10, 24, 25, 64):
            assert BC.lstm_step_ok(B, H) == K.lstm_step_ok(B, H)
    for n_out in (1, 3):
        hmid, w1 = torch.zeros(7, 8), torch.zeros(n_out, 8)
        assert BC.rowdot_ok_sizes(n_out) == (n_out == 1 and K.rowdot_ok(hmid, w1))
    assert K.LEAKY_SLOPE == BC.SLOPE


@pytest.mark.parametrize('name', [n for n in sorted(BC.CACHE_CASES) if n != 'lstm'])
def test_weight_caches_follow_the_parameters(model, name):
    fam = BC.FAMILIES[name]
    for i in BC.CACHE_CASES[name]:
        case = fam.cases()[i]
        if BC.is_f32(case):         # (the bf16 images are GPU-only: the model has no bf16 storage)
            BC.check_cache(fam, case, 'cpu', BC.cache_floors(fam, case))
            BC.check_changed_between(fam, case, 'cpu')


def test_bce_backward_without_a_gradient(model):
    BC.bce_backward_without_gradient()


def test_the_checker_notices_a_changed_second_run_and_a_stray_gradient(model, floors):
    fam = BC.FAMILIES['dhead']
    case = fam.cases()[4]
    got, ref = BC.run_block(fam, case, 'fresh', 'cpu'), BC.ref_block(fam, case, 'fresh')
    other = dict(got, outs=[got['outs'][0].clone()])
    other['outs'][0][0, 0] += 1e-7
    with pytest.raises(AssertionError, match='not reproducible'):
        BC.check_block(fam, case, 'fresh', got, ref, floors['dhead'][(case['id'], 'fresh')], again=other)
    fr, refz = BC.run_block(fam, case, 'frozen', 'cpu'), BC.ref_block(fam, case, 'frozen')
    fr['grads'][2] = fr['grads'][2] + 1e-6
    with pytest.raises(AssertionError, match='frozen: .grad touched'):
        BC.check_routes(fam, case, dict(fresh=got, frozen=fr))
    del refz


# ---------------------------------------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------------------------------------
def _m_axpby_skipped(mp, K):
    """1. the gradient of an intermediate DConvStackFn output is dropped"""
    fired = []
    mp.setattr(K, 'axpby', lambda x, y, a, b: fired.append(1))
    return fired


def _m_gate_lens_of_layer_i(mp, K):
    """2. the gated epilogue masks with layer i's lengths instead of layer i - 1's"""
    real, fired = K.conv_engine, []

    def conv_engine(x, wp, y, K_, stride, pad, mode, bias=None, res=None, lens=None, act=0, **kw):
        if act == K.ACT_LEAKY_GATE and lens is not None:
            fired.append(1)
            ll = BC.LAST['lens_list']
            j = [i for i, l in enumerate(ll) if l is lens]
            assert len(j) == 1 and j[0] + 1 < len(ll)
            lens = ll[j[0] + 1]
        return real(x, wp, y, K_, stride, pad, mode, bias, res, lens, act, **kw)
    mp.setattr(K, 'conv_engine', conv_engine)
    return fired


def _m_no_add_into(mp, K):
    """3. GTrunkFn loses add_into (the dense residual gradient)"""
    real, fired = K.leaky_bwd, []
    mp.setattr(K, 'leaky_bwd', lambda dy, y, dpre, lens=None, add_into=None, bias_grad=None, **kw:
               (fired.append(1) if add_into is not None else None, real(dy, y, dpre, lens=lens, bias_grad=bias_grad, **kw))[1])
    return fired


def _m_fold_without_identity(mp, K):
    """4. DHeadFn 'fold' runs without the identity"""
    from audiogan_amd import ops
    fired = []
    mp.setattr(ops, '_eye', lambda w: (fired.append(1), torch.zeros_like(w))[1])
    return fired


def _m_reverse_dwhh_same_time(mp, K):
    """5. the reverse direction's dw_hh is paired with the same-time y instead of the next step's"""
    from audiogan_amd import ops
    real, fired = ops._prod, []

    def _prod(A, Bm, out, **k):
        off, pitch = Bm.storage_offset(), Bm.stride(0)
        if k.get('ta') and Bm.dim() == 2 and Bm.size(1) < pitch and off >= pitch:      # y2[B:, H:2H]: rows one step later
            Bm = Bm.as_strided(Bm.shape, Bm.stride(), off - off // pitch * pitch)
            fired.append(1)
        return real(A, Bm, out, **k)
    mp.setattr(ops, '_prod', _prod)
    return fired


def _m_dstatic_one_direction(mp, K):
    """6. dstatic is taken from one direction only"""
    real, fired = K.gemm, []

    def gemm(A, Bm, Cm, ta=False, tb=False, alpha=1.0, beta=0.0, **k):
        if beta == 1.0 and not ta and not tb and Bm.storage_offset() > 0 and Bm.stride(0) > Bm.size(1) and bool(Cm.any()):
            fired.append(1)
            return None                        # (the static columns of W_ih, into a dstatic that already holds direction 0)
        return real(A, Bm, Cm, ta=ta, tb=tb, alpha=alpha, beta=beta, **k)
    mp.setattr(K, 'gemm', gemm)
    return fired


def _m_wn_backward_overwrites(mp, K):
    """7. WNGroup.backward overwrites .grad instead of accumulating"""
    real, fired = K.weight_norm_bwd, []
    mp.setattr(K, 'weight_norm_bwd', lambda ents: (fired.extend(1 for e in ents if e.get('accumulate')),
                                                   real([dict(e, accumulate=False) for e in ents]))[1])
    return fired


def _m_prepare_ignores_epoch(mp, K):
    """8. prepare() ignores the parameter epoch"""
    from audiogan_amd import common
    fired = []
    mp.setattr(common, 'param_epoch', lambda p: (fired.append(1), 0)[1])
    return fired


def _m_second_backward_skips_finish(mp, K):
    """9. the second backward in a scope skips finish_pending"""
    from audiogan_amd import common
    fired = []
    mp.setattr(common, 'finish_pending', lambda: fired.append(1))
    return fired


def _m_backward_time_freeze_ignored(mp, K):
    """10. WNGroup.backward does not look at requires_grad when the backward runs (the stopper-only backward)"""
    from audiogan_amd import common
    real, fired = common.WNGroup.backward, []

    def backward(self, dws, needs=None):
        ps = [p for p in self.params() if not p.requires_grad]
        fired.extend(ps)
        for p in ps:
            p.requires_grad_(True)
        try:
            return real(self, dws, needs)
        finally:
            for p in ps:
                p.requires_grad_(False)
    mp.setattr(common.WNGroup, 'backward', backward)
    return fired


def _m_forward_time_freeze_ignored(mp, K):
    """11. WNGroup.backward does not look at what required a gradient when the forward ran (a forward under frozen)"""
    from audiogan_amd import common
    real, fired = common.WNGroup.backward, []

    def backward(self, dws, needs=None):
        fired.extend(1 for n in (needs or ()) if not n)
        return real(self, dws, None)
    mp.setattr(common.WNGroup, 'backward', backward)
    return fired


MUTANTS = [(_m_axpby_skipped, 'dconv', 'sweep', r'out of bound: (dx|d\.l)'),
           (_m_gate_lens_of_layer_i, 'dconv', 'sweep', r'out of bound: (dx|d\.l)'),
           (_m_no_add_into, 'gtrunk', 'sweep', r'out of bound: (dx|d\.bn)'),
           (_m_fold_without_identity, 'dhead', 'sweep', r'out of bound: (dx|d\.res)'),
           (_m_reverse_dwhh_same_time, 'lstm', 'sweep', r'out of bound: d\.d1\.w_hh'),
           (_m_dstatic_one_direction, 'lstm', 'sweep', r'out of bound: dx1'),
           (_m_wn_backward_overwrites, 'gtrunk', 'sweep', r'out of bound: d\.|route changes bits'),
           (_m_wn_backward_overwrites, 'dhead', 'sweep', r'out of bound: d\.|route changes bits'),
           (_m_prepare_ignores_epoch, 'gtrunk', 'cache', r'stale weights after a parameter changed \(optim\)'),
           (_m_prepare_ignores_epoch, 'dconv', 'cache', r'stale weights after a parameter changed \(optim\)'),
           (_m_prepare_ignores_epoch, 'dhead', 'cache', r'stale weights after a parameter changed \(optim\)'),
           (_m_second_backward_skips_finish, 'gtrunk', 'sweep', r'out of bound: d\.'),
           (_m_second_backward_skips_finish, 'dconv', 'sweep', r'out of bound: d\.'),
           (_m_second_backward_skips_finish, 'dhead', 'sweep', r'out of bound: d\.'),
           (_m_backward_time_freeze_ignored, 'gtrunk', 'sweep', r'out of bound: d\.|partly frozen \(part_bwd\w*\): .grad touched'),
           (_m_backward_time_freeze_ignored, 'dconv', 'sweep', r'out of bound: d\.|partly frozen \(part_bwd\w*\): .grad touched'),
           (_m_backward_time_freeze_ignored, 'dhead', 'sweep', r'out of bound: d\.|partly frozen \(part_bwd\w*\): .grad touched'),
           (_m_forward_time_freeze_ignored, 'gtrunk', 'sweep', r'out of bound: d\.|partly frozen \(part_fwd\w*\): .grad touched'),
           (_m_forward_time_freeze_ignored, 'dconv', 'sweep', r'out of bound: d\.|partly frozen \(part_fwd\w*\): .grad touched'),
           (_m_forward_time_freeze_ignored, 'dhead', 'sweep', r'out of bound: d\.|partly frozen \(part_fwd\w*\): .grad touched')]


@pytest.mark.parametrize('mutant,name,what,trips', MUTANTS, ids=['%s-%s' % (m.__name__[3:], n) for m, n, _, _ in MUTANTS])
def test_the_sweep_rejects_a_mutant(model, monkeypatch, floors, mutant, name, what, trips):
    fam = BC.FAMILIES[name]
    if what == 'cache':
        case = fam.cases()[BC.CACHE_CASES[name][0]]
        fl = BC.cache_floors(fam, case)
    fired = mutant(monkeypatch, model)
    try:
        if what == 'cache':
            BC.check_cache(fam, case, 'cpu', fl)
        else:
            BC.sweep(fam, 'cpu', floors[name])
    except AssertionError as e:
        msg = str(e)
    else:
        assert fired, 'the mutant never fired: the call it patches is no longer recognised (%s)' % mutant.__doc__
        raise AssertionError('the sweep accepted a mutant: ' + mutant.__doc__)
    assert fired, 'the mutant never fired: the sweep failed for another reason (%s): %s' % (mutant.__doc__, msg[:300])
    assert re.search(trips, msg), (mutant.__doc__, msg[:300])


def test_each_mutant_is_rejected_by_the_route_or_case_meant_for_it(model, monkeypatch, floors):
    """the mutants that live on ONE route or structural class are invisible elsewhere: the sweep needs that route / class"""
    fam = BC.FAMILIES['dhead']
    with monkeypatch.context() as mp:
        _m_second_backward_skips_finish(mp, model)
        fl = {k: v for k, v in floors['dhead'].items()}
        for case in BC.host_cases(fam):     # every route but 'twice' passes
            for r in [r for r in fam.routes if not BC.ROUTE[r]['twice']]:
                BC.check_block(fam, case, r, BC.run_block(fam, case, r, 'cpu'), BC.ref_block(fam, case, r), fl[(case['id'], r)])
    with monkeypatch.context() as mp:
        _m_fold_without_identity(mp, model)
        for case in [c for c in BC.host_cases(fam) if c['n_res'] < 2]:     # the identity is folded only above residual 0
            BC.check_block(fam, case, 'fresh', BC.run_block(fam, case, 'fresh', 'cpu'), BC.ref_block(fam, case, 'fresh'),
                           floors['dhead'][(case['id'], 'fresh')])
    fam = BC.FAMILIES['dconv']
    with monkeypatch.context() as mp:
        _m_axpby_skipped(mp, model)
        for case in [c for c in BC.host_cases(fam) if sum(c['pat']) == 1]:  # one gradient: nothing to add
            BC.check_block(fam, case, 'fresh', BC.run_block(fam, case, 'fresh', 'cpu'), BC.ref_block(fam, case, 'fresh'),
                           floors['dconv'][(case['id'], 'fresh')])
