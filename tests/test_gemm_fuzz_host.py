"""The GEMM dispatch fuzz (tests/gemm_cases.py) against the CPU model of the kernels: the generator, runner, reference and
checker that tests/test_gemm_fuzz.py turns on the HIP kernels are shown here, without a GPU, to (a) accept a correct
implementation of the contract and (b) REJECT implementations that are subtly wrong - each mutant below is a mistake a
GEMM kernel can make on one path (a dropped k element or K slice, an epilogue branch, a write outside the window, a wrong
rounding).  It also shows, on sizes alone, that the seeded case lists hold the shape classes the GPU coverage assertions
need (the GPU test asserts them again on the kernel names the library reports)."""
import pytest
import torch

from tests import gemm_cases as GC
from tests import kernel_model as KM

SMALL = 1.2e8          # M N K of the reduced list: the CPU model's fp32 products stay below a second in all


def _trunc(t):
    """round toward zero to bf16 precision (the WRONG rounding), kept in fp32"""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def model(mode, mutate=None):
    """kernels.gemm as the CPU model computes it in precision `mode`"""
    def fn(A, B, Cm, **kw):
        if mode == 'bf16':
            A, B = (_trunc(A), _trunc(B)) if mutate == 'truncate' else (A.bfloat16().float(), B.bfloat16().float())
        _mutated(KM.gemm, mutate, A, B, Cm, **kw)
    return fn


def model_h(mutate=None):
    """kernels.gemm_h from the model's gemm: bf16 operands / residual as their fp32 values, gate16 after the epilogue, the
    bf16 output rounded to nearest even"""
    def fn(A, B, C=None, C16=None, gate=None, res=None, **kw):
        out = C if C is not None else torch.full(tuple(C16.shape), float('nan'))
        _mutated(KM.gemm, None if mutate == 'stray_write' else mutate, A.float(), B.float(), out,
                 res=res.float() if res is not None else None, **kw)
        if gate is not None:
            out.copy_(torch.where(gate.float() > 0, out, out * kw['slope']))
        if C16 is not None:
            C16.copy_(_trunc(out).bfloat16() if mutate == 'truncate' else out.bfloat16())
        if mutate == 'stray_write':
            _stray(C16 if C16 is not None else C)
    return fn


def _stray(Cm):
    """one write to the element right behind the last one of the window"""
    M, N = Cm.shape
    Cm.as_strided((1,), (1,), Cm.storage_offset() + (M - 1) * Cm.stride(0) + N).fill_(1.0)


def _mutated(gemm, mutate, A, B, Cm, **kw):
    ta, tb = kw['ta'], kw['tb']
    M, N = Cm.shape
    Kd = A.size(0) if ta else A.size(1)

    def zero_k_from(k0):
        a = A.clone()
        if ta:
            a[k0:] = 0
        else:
            a[:, k0:] = 0
        return a
    if mutate == 'last_k':
        A = zero_k_from(Kd - 1)
    elif mutate == 'last_slice':
        plan = GC.gemm_plan('f32', M, N, Kd, int(ta), int(tb), GC.opts(), act=kw['act'])
        if plan['ksplit'] > 1:
            A = zero_k_from((plan['ksplit'] - 1) * plan['kchunk'])
    elif mutate == 'no_beta':
        kw = dict(kw, beta=0.0)
    elif mutate == 'gate_adds_res' and kw['act'] == GC.ACT_LEAKY_GATE:
        kw = dict(kw, act=GC.ACT_NONE)
    before = Cm.clone()
    gemm(A, B, Cm, **kw)
    if mutate == 'reads_c' and kw['beta'] == 0.0:
        Cm.copy_(Cm + 0.0 * before)
    if mutate == 'stray_write':
        _stray(Cm)


@pytest.fixture(scope='module')
def prepared():
    """inputs and float64 references of the reduced lists, computed once: {(h, index, pass name): (case, pas, inp, ref)}"""
    out = {}
    for h, lst in ((False, GC.cases()), (True, GC.cases_h())):
        for ci, case in enumerate(lst):
            if case[0] * case[1] * case[2] > SMALL:
                continue
            for pas in (GC.EXACT, GC.REAL):
                inp = GC.make_inputs(case, pas, 1000 + ci, h=h)
                out[(h, ci, pas['name'])] = (case, pas, inp, GC.reference(case, pas, inp), )
    return out


def _sweep(prepared, mode, fn):
    h = mode == 'h'
    for (h_, ci, _), (case, pas, inp, ref) in prepared.items():
        if h_ != h:
            continue
        full = None
        if mode == 'bf16':
            full, ref = ref, GC.reference(case, pas, inp, rounded=True)
            if pas is GC.EXACT:
                full = None
        got = GC.run(fn, case, pas, inp, 'cpu', h=h)
        GC.check(case, pas, mode, ref, got, full=full)


@pytest.mark.parametrize('mode', ['f32', 'bf16', 'h'])
def test_checker_accepts_the_model(prepared, mode):
    _sweep(prepared, mode, model_h() if mode == 'h' else model(mode))


@pytest.mark.parametrize('mode,mutate', [('f32', 'last_k'), ('f32', 'last_slice'), ('f32', 'no_beta'), ('f32', 'reads_c'),
                                         ('f32', 'gate_adds_res'), ('f32', 'stray_write'), ('bf16', 'truncate'),
                                         ('h', 'last_k'), ('h', 'stray_write'), ('h', 'truncate')])
def test_checker_rejects_a_mutant(prepared, mode, mutate):
    with pytest.raises(AssertionError):
        _sweep(prepared, mode, model_h(mutate) if mode == 'h' else model(mode, mutate))


def test_each_pass_rejects_a_dropped_k_element_on_its_own(prepared):
    """zero tolerance on integers and the declared bound on randn operands each catch one missing product term"""
    for pas_name in ('exact', 'real'):
        one = {k: v for k, v in prepared.items() if k[2] == pas_name}
        with pytest.raises(AssertionError):
            _sweep(one, 'f32', model('f32', 'last_k'))


def test_case_lists_are_seeded_and_hold_the_shape_classes_the_gpu_coverage_needs():
    lst, lst_h = GC.cases(), GC.cases_h()
    assert lst == GC.cases() and lst_h == GC.cases_h(), 'the generator is not deterministic'
    assert len(lst) >= 60 and len(lst_h) >= 60
    for l in (lst, lst_h):
        total = sum(float(c[0]) * c[1] * c[2] for c in l)
        assert total <= 2.5e10 and max(c[0] * c[1] * c[2] for c in l) <= GC.MNK_MAX, total
        assert all(c[2] <= 8192 for c in l), 'the exactness argument of the integer pass needs K <= 8192'
    assert all(GC.gemm_h_ok(*c[:5]) for c in lst_h)
    # named by the issue: the bf16-mode fallback onto the 128-tile fp32 kernel, split-eligible cases in all four layouts
    assert any(c[0] > 64 and c[1] > 64 and c[2] >= 2048 and c[2] % 4 != 0 for c in lst)
    for l in GC.LAYOUTS:
        assert any((c[3], c[4]) == l and GC.split_eligible(c[0], c[1], c[2], c[5]['act']) for c in lst)
    # the whole coverage list of the GPU tests, on the dispatch restated on sizes
    for mode in ('f32', 'bf16', 'f32x3'):
        GC.assert_gemm_coverage(mode, [(c, GC.gemm_plan(mode, *c)['kernel'], GC.split_eligible(c[0], c[1], c[2], c[5]['act']))
                                       for c in lst])
    GC.assert_gemm_h_coverage([(c, GC.gemm_h_plan(*c)['kernel'], GC.gemm_h_plan(*c)['eligible']) for c in lst_h])


def test_coverage_assertion_fails_when_a_form_is_not_reached():
    lst = GC.cases()

    def seen(l, mode='f32'):
        return [(c, GC.gemm_plan(mode, *c)['kernel'], GC.split_eligible(c[0], c[1], c[2], c[5]['act'])) for c in l]
    with pytest.raises(AssertionError):
        GC.assert_gemm_coverage('f32', seen([c for c in lst if c[2] < 2048]))                  # no 128-tile kernel at all
    with pytest.raises(AssertionError):
        GC.assert_gemm_coverage('f32', seen([c for c in lst if c[5]['act'] != GC.ACT_TANH]))   # tanh never on a DMA interior tile
    with pytest.raises(AssertionError):
        GC.assert_gemm_coverage('f32', seen([c for c in lst if not (c[5]['view'] and c[2] >= 1024)]))   # no split into a pitched C
    with pytest.raises(AssertionError):
        GC.assert_gemm_h_coverage([(c, GC.gemm_h_plan(*c)['kernel'], GC.gemm_h_plan(*c)['eligible'])
                                   for c in GC.cases_h() if not c[5]['res16']])


def test_large_tile_shapes_select_their_tiles():
    for (M, N, K), tile in GC.LARGE_TILES:
        for ta, tb in GC.LAYOUTS:
            assert GC.gemm_plan('f32', M, N, K, ta, tb, GC.opts(view=1))['kernel'] == \
                'gemm_tile_kernel<%d,%d,%d,%d,%d,%d>' % ((ta, tb) + tile)
            assert GC.has_interior(M, N, *tile[:2]) and M % tile[0] and N % tile[1]
