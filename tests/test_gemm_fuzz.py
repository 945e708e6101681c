"""-m gpu: the dense products (ag_gemm in its three precision modes, ag_gemm_h) walked through their dispatch space against
float64 - every kernel form (64-tile / 128-tile register-staged gemm_kernel, the four LDS-DMA tiles of gemm_tile_kernel,
gemm_bf16_kernel plain and split-bf16, gemm_bf16s_kernel; 36 instantiations), interior and ragged epilogues, vector and
scalar loaders, split-K with its second stages (stand-alone, short workspace, none, deferred), every epilogue option on its
own and combined, pitched and unaligned views, and a sentinel frame around every output.

Two passes per case (tests/gemm_cases.py): integer operands, where every result must equal the float64 reference bit for
bit, and randn operands under the project's declared bounds.  After each list the coverage lists
assert which kernels (by the name the library reports) and which paths were reached; tests/test_gemm_fuzz_host.py shows on
the CPU model that the checker rejects subtly wrong products."""
import ctypes as C

import pytest
import torch

from tests import gemm_cases as GC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    return K_


def _last(K):
    return lambda: K.lib.ag_last_kernel().decode()


def _both_passes(K, fn, case, ci, mode, h=False, rerun=False, **extra):
    """one case through `fn`, both passes; returns (kernel name, the real pass's error as a fraction of the scale)"""
    err = 0.0
    for pas in (GC.EXACT, GC.REAL):
        inp = GC.make_inputs(case, pas, 1000 + ci, h=h)
        ref = GC.reference(case, pas, inp, rounded=mode == 'bf16')
        full = GC.reference(case, pas, inp) if (mode == 'bf16' and pas is GC.REAL and case[2] >= 36) else None
        got = GC.run(fn, case, pas, inp, 'cuda', h=h, last_kernel=_last(K), **extra)
        err = GC.check(case, pas, mode, ref, got, full=full)
        if rerun:                     # a two-stage product sums its slabs in a fixed order
            again = GC.run(fn, case, pas, inp, 'cuda', h=h, last_kernel=_last(K), **extra)
            assert torch.equal(again['c'], got['c']) and again['kernel'] == got['kernel'], ('not reproducible', case, pas['name'])
    return got['kernel'], err


@pytest.mark.parametrize('mode', ['f32', 'bf16', 'f32x3'])
def test_gemm_random_cases(K, mode):
    seen, worst = [], 0.0
    with K.precision(mode):
        for ci, case in enumerate(GC.cases()):
            M, N, Kd, ta, tb, o = case
            split = K.lib.ag_gemm_ws_numel(M, N, Kd, o['act']) > 0
            name, err = _both_passes(K, K.gemm, case, ci, mode, rerun=split)
            seen.append((case, name, split))
            worst = max(worst, err)
    print('gemm fuzz, %s mode: largest real-pass error %.3g of the scale' % (mode, worst))
    GC.assert_gemm_coverage(mode, seen)


def test_gemm_h_random_cases(K):
    seen, worst = [], 0.0
    for ci, case in enumerate(GC.cases_h()):
        M, N, Kd, ta, tb, o = case
        eligible = (not o['gate']) and K.lib.ag_gemm_h_ws_numel(M, N, Kd, o['act'], int(o['out'] != 'c')) > 0
        name, err = _both_passes(K, K.gemm_h, case, ci, 'h', h=True, rerun=eligible)
        seen.append((case, name, eligible))
        worst = max(worst, err)
    print('gemm_h fuzz: largest real-pass error of the fp32 output %.3g of the scale' % worst)
    GC.assert_gemm_h_coverage(seen)


@pytest.mark.parametrize('ta,tb', GC.LAYOUTS)
@pytest.mark.parametrize('ti', [0, 1, 2])
def test_gemm_large_tiles(K, ti, ta, tb):
    """256 x 128, 128 x 256 and 256 x 256 of gemm_tile.h as gemm_pick_tile selects them (confirmed by the kernel name), ragged
    in both directions, into a pitched C inside a sentinel frame; one layout per tile also runs bias + res + beta + tanh
    through the interior epilogue"""
    (M, N, Kd), tile = GC.LARGE_TILES[ti]
    want = 'gemm_tile_kernel<%d,%d,%d,%d,%d,%d>' % ((ta, tb) + tile)
    with K.precision('f32'):
        name, _ = _both_passes(K, K.gemm, (M, N, Kd, ta, tb, GC.opts(alpha=1, bias=1, view=1)), 50 + ti, 'f32')
        assert name == want, (name, want)
        if GC.LAYOUTS[ti] == (ta, tb):
            o = GC.opts(alpha=2, beta=2, bias=1, res=1, act=GC.ACT_TANH, view=1)
            name, _ = _both_passes(K, K.gemm, (M, N, Kd, ta, tb, o), 60 + ti, 'f32')
            assert name == want, (name, want)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _raw_gemm(K, A, B, Cw, M, N, Kd, ta, tb, alpha, beta, bias, res):
    """ag_gemm itself: whatever ag_bind_workspace bound before is what the call finds"""
    return K.lib.ag_gemm(_ptr(A), A.stride(0), ta, _ptr(B), B.stride(0), tb, _ptr(Cw), Cw.stride(0), M, N, Kd, alpha, beta,
                         _ptr(bias), _ptr(res), res.stride(0) if res is not None else 0, GC.ACT_NONE, 0.0,
                         C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_gemm_split_k_workspace_sizes(K):
    """a split-eligible product with ragged tiles under the full workspace (16 slices), one for two slices, one for three and
    a bit (fewer slices than wanted), and none (the header: "runs unsplit"): exact on integers, within the bound on randn
    operands, every time; a workspace bound for a call that fails its argument check is gone for the next call"""
    M, N, Kd, ta, tb = 200, 132, 4096, 1, 0
    case = (M, N, Kd, ta, tb, GC.opts(alpha=1, beta=2, bias=1, res=1, view=1))
    full = K.lib.ag_gemm_ws_numel(M, N, Kd, GC.ACT_NONE)
    assert full == 16 * M * N
    with K.precision('f32'):
        for pas in (GC.EXACT, GC.REAL):
            inp = GC.make_inputs(case, pas, 7)
            ref = GC.reference(case, pas, inp)
            for numel in (full, 2 * M * N, 3 * M * N + 5, 0):
                ws = torch.empty(max(numel, 4), device='cuda')

                def fn(A, B, Cw, ta, tb, alpha, beta, bias, res, act, slope):
                    if numel:
                        assert K.lib.ag_bind_workspace(_ptr(ws), numel) == 0
                    else:
                        K.lib.ag_bind_workspace(None, 0)
                    fn.err = K.lib.ag_last_error()
                    assert _raw_gemm(K, A, B, Cw, M, N, Kd, int(ta), int(tb), alpha, beta, bias, res) == 0, K.lib.ag_last_error()
                    assert K.lib.ag_last_error() == fn.err, 'a product without a workspace is no error'
                got = GC.run(fn, case, pas, inp, 'cuda', last_kernel=_last(K))
                GC.check(case, pas, 'f32', ref, got)
                assert got['kernel'] == 'gemm_tile_kernel<1,0,128,128,2,2>', got['kernel']
        # the binding is taken FIRST: an argument error must not leave it to the next call
        inp = GC.make_inputs(case, GC.EXACT, 7)
        ws = torch.full((full,), GC.SENTINEL, device='cuda')

        def fn2(A, B, Cw, ta, tb, alpha, beta, bias, res, act, slope):
            assert K.lib.ag_bind_workspace(_ptr(ws), full) == 0
            assert _raw_gemm(K, A, B, Cw, 0, N, Kd, int(ta), int(tb), alpha, beta, bias, res) == -1
            assert b'bad shape' in K.lib.ag_last_error()
            assert _raw_gemm(K, A, B, Cw, M, N, Kd, int(ta), int(tb), alpha, beta, bias, res) == 0
        got = GC.run(fn2, case, GC.EXACT, inp, 'cuda', last_kernel=_last(K))
        GC.check(case, GC.EXACT, 'f32', GC.reference(case, GC.EXACT, inp), got)
        assert bool((ws == GC.SENTINEL).all()), 'the call after a failed one found the failed call\'s workspace'


@pytest.mark.parametrize('ta,tb', GC.LAYOUTS)
def test_gemm_deferred_second_stage_layouts(K, ta, tb):
    """a ragged split-K product into a pitched C with defer=True inside a deferral scope, beta 0 and 1: nothing is written
    before the flush; afterwards the result equals the stand-alone call bit for bit (exact on integers), and the columns
    outside the view are untouched"""
    M, N, Kd = 200, 132, 2048
    with K.precision('f32'):
        for pas in (GC.EXACT, GC.REAL):
            cases = [(M, N, Kd, ta, tb, GC.opts(alpha=1, beta=b, view=1)) for b in (0, 1)]
            assert K.lib.ag_gemm_ws_numel(M, N, Kd, GC.ACT_NONE) > 0
            inps = [GC.make_inputs(c, pas, 70 + i) for i, c in enumerate(cases)]
            alone = [GC.run(K.gemm, c, pas, i, 'cuda', last_kernel=_last(K)) for c, i in zip(cases, inps)]
            for c, i, g in zip(cases, inps, alone):
                GC.check(c, pas, 'f32', GC.reference(c, pas, i), g)
            with K.deferred_reduces():
                inside = [GC.run(K.gemm, c, pas, i, 'cuda', last_kernel=_last(K), defer=True) for c, i in zip(cases, inps)]
                torch.cuda.synchronize()
                assert bool(torch.isnan(inside[0]['c']).all()), 'beta = 0: the deferred second stage ran before the flush'
                assert torch.equal(inside[1]['c'], inps[1]['C0']), 'beta = 1: the deferred second stage ran before the flush'
            torch.cuda.synchronize()
            for g, d in zip(alone, inside):
                frame = d['frames'][0]
                assert torch.equal(frame.window(), g['c']), 'deferred and stand-alone second stages differ'
                assert frame.untouched()
