"""-m gpu: the convolution path walked through its dispatch space against float64 - the conv engine (six tile
configurations, both tail pairings, the ten tap specialisations, generic / register-pipelined / solo / solo + DMA staging,
the bf16 kernel with NW 8 and 16 and its fall-backs, aligned and unaligned scatter layouts, the single-channel streaming
kernels and each reason they are declined, every epilogue option alone and combined), the weight gradient (three MFMA
tiles in fp32 and bf16, each refusal of the bf16 kernel, time chunks and slice counts, halos, accumulation into a non-zero
dw, the single-channel kernels, short workspaces) and the companions of a layer's backward (channel_sum, leaky_bwd,
conv_o1_*), in fp32 and bf16 mode.

Two passes per case (tests/conv_cases.py): integer operands, where every output must equal the float64 reference bit for
bit, and randn operands under the bound rule of DESIGN.md section 2 (16 x the fp32 CPU model's own error, never above 1e-4
of the output scale).  Every output sits in a sentinel-filled frame that must come back untouched; two-stage reductions run
twice for identical bits.  The kernel name the library reports is asserted equal to the restated dispatch for every case,
and each test ends in coverage assertions on those names and on the plan classes.  The 40 seeded shapes of the earlier
version of this file (forward, backward-data, backward-weight) are part of the lists.  tests/test_conv_fuzz_host.py shows on
the CPU model that the checker rejects subtly wrong kernels.  Each test prints the largest real-pass error / floor per
kernel form (pytest -s)."""
import ctypes as C

import pytest
import torch

from tests import conv_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    return K_


def test_constants_restated_in_the_case_module_match_the_library(K):
    """tests/conv_cases.py states the activation codes, the slope and the wrappers' small workspace itself (it is imported
    by the host test, which has no library): a drift would otherwise show only indirectly, and for the kernels that report no
    name not at all"""
    assert (CC.ACT_NONE, CC.ACT_LEAKY, CC.ACT_TANH, CC.ACT_LEAKY_GATE) == (K.ACT_NONE, K.ACT_LEAKY, K.ACT_TANH, K.ACT_LEAKY_GATE)
    assert CC.LEAKY_SLOPE == K.LEAKY_SLOPE and CC.REAL['slope'] == K.LEAKY_SLOPE
    assert CC.SMALL_WS == K._SMALL_WS


def _last(K):
    return lambda: K.lib.ag_last_kernel().decode()


def _report(what, prec, worst):
    print('conv fuzz, %s, %s mode: largest real-pass error / floor per kernel form' % (what, prec))
    for form in sorted(worst):
        print('  %-44s %6.2f' % (form, worst[form]))


def _form(pl):
    return pl['kernel'] + ' ' + pl['form']


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_conv_engine_cases(K, prec):
    seen, worst = [], {}
    with K.precision(prec):
        for ci, (label, c) in enumerate(CC.engine_cases()):
            pl = CC.conv_plan(prec, c)
            for pas in (CC.EXACT, CC.REAL):
                inp = CC.engine_inputs(c, pas, 1000 + ci)
                ref = CC.engine_reference(c, pas, inp, rounded=prec == 'bf16')
                floor = CC.engine_floor(c, pas, inp, rounded=prec == 'bf16') if pas is CC.REAL else None
                got = CC.run_engine(K, c, pas, inp, 'cuda', last_kernel=_last(K))
                assert got['kernel'] == pl['kernel'], ('the restated dispatch and the library disagree', label, c, got['kernel'], pl['kernel'])
                ratio = CC.check((label, c), pas, ref, got, floor=floor, form=_form(pl), output='y')
                worst[_form(pl)] = max(worst.get(_form(pl), 0.0), ratio)
            seen.append((label, c, got['kernel'], pl))
    _report('engine', prec, worst)
    CC.assert_engine_coverage(prec, seen)


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_conv_wgrad_cases(K, prec):
    seen, worst = [], {}
    with K.precision(prec):
        for ci, (label, c) in enumerate(CC.wgrad_cases()):
            pl = CC.wgrad_plan(prec, c)
            assert K.lib.ag_conv1d_wgrad_ws_numel(c.B, c.A, c.Lsh, c.C, c.K) == pl['ws_want'], (label, c)
            for pas in (CC.EXACT, CC.REAL):
                inp = CC.wgrad_inputs(c, pas, 1000 + ci)
                ref = CC.wgrad_reference(c, pas, inp, rounded=prec == 'bf16')
                floor = CC.wgrad_floor(c, pas, inp, rounded=prec == 'bf16') if pas is CC.REAL else None
                got = CC.run_wgrad(K, c, pas, inp, 'cuda', last_kernel=_last(K))
                again = CC.run_wgrad(K, c, pas, inp, 'cuda', last_kernel=_last(K))      # two-stage, fixed order
                assert got['kernel'] == pl['kernel'], ('the restated dispatch and the library disagree', label, c, got['kernel'], pl['kernel'])
                ratio = CC.check((label, c), pas, ref, got, floor=floor, form=pl['kernel'], output='dw', again=again)
                worst[pl['kernel']] = max(worst.get(pl['kernel'], 0.0), ratio)
            seen.append((label, c, got['kernel'], pl))
    _report('weight gradient', prec, worst)
    CC.assert_wgrad_coverage(prec, seen)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def test_conv_wgrad_workspace_sizes(K):
    """the slice count is capped by the bound workspace: the full one (16 slabs), three slabs and a bit, exactly one slab -
    the result is right every time, exact on integers - and below one slab the documented argument error, after which the
    next call does not find the failed call's binding"""
    c = CC.WS_CASE
    n_out = c.A * c.C * c.K
    full = K.lib.ag_conv1d_wgrad_ws_numel(c.B, c.A, c.Lsh, c.C, c.K)
    assert full == CC.wgrad_plan('f32', c)['ws_want'] and full // n_out > 3
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(numel, ws):
        def call(sh, lg, dw, K_, s, p):
            if numel:
                assert K.lib.ag_bind_workspace(_ptr(ws), numel) == 0
            else:
                K.lib.ag_bind_workspace(None, 0)
            call.rc = K.lib.ag_conv1d_wgrad(_ptr(sh), sh.stride(0), sh.stride(1), _ptr(lg), lg.stride(0), lg.stride(1), _ptr(dw),
                                            c.B, c.A, c.Lsh, c.C, c.Llg, K_, s, p, stream)
            call.err = K.lib.ag_last_error()
        return call
    with K.precision('f32'):
        for pas in (CC.EXACT, CC.REAL):
            inp = CC.wgrad_inputs(c, pas, 7)
            ref, floor = CC.wgrad_reference(c, pas, inp), CC.wgrad_floor(c, pas, inp)
            for numel in (full, 3 * n_out + 5, n_out):
                ws = torch.full((numel + 64,), CC.SENTINEL, device='cuda')
                call = raw(numel, ws)
                got = CC.run_wgrad(K, c, pas, inp, 'cuda', last_kernel=_last(K), call=call)
                assert call.rc == 0, call.err
                assert got['kernel'] == 'conv_wgrad_kernel<2,2,2,2>'
                CC.check(('workspace', numel), pas, ref, got, floor=floor, form=got['kernel'], output='dw')
                assert bool((ws[numel:] == CC.SENTINEL).all()), 'wrote past the bound workspace'
                used = CC.wgrad_plan('f32', c, numel)['gz'] * n_out
                assert bool((ws[used:numel] == CC.SENTINEL).all()), 'more slabs written than the plan says'
        # below one slab, and none at all: the documented error, dw untouched
        inp = CC.wgrad_inputs(c, CC.EXACT, 7)
        for numel in (n_out - 1, 0):
            ws = torch.full((n_out + 64,), CC.SENTINEL, device='cuda')
            call = raw(numel, ws)
            got = CC.run_wgrad(K, c, CC.EXACT, inp, 'cuda', call=call)
            assert call.rc == -1 and b'needs a workspace of >= %d floats' % n_out in call.err, (call.rc, call.err)
            assert torch.equal(got['out'], inp['dw0']) and got['frame_ok']
            assert bool((ws == CC.SENTINEL).all())
        # the binding is taken FIRST: an argument error must not leave it to the next call
        ws = torch.full((full,), CC.SENTINEL, device='cuda')

        def call2(sh, lg, dw, K_, s, p):
            assert K.lib.ag_bind_workspace(_ptr(ws), full) == 0
            rc = K.lib.ag_conv1d_wgrad(_ptr(sh), sh.stride(0), sh.stride(1), _ptr(lg), lg.stride(0), lg.stride(1), _ptr(dw),
                                       0, c.A, c.Lsh, c.C, c.Llg, K_, s, p, stream)
            assert rc == -1 and b'bad shape' in K.lib.ag_last_error()
            rc = K.lib.ag_conv1d_wgrad(_ptr(sh), sh.stride(0), sh.stride(1), _ptr(lg), lg.stride(0), lg.stride(1), _ptr(dw),
                                       c.B, c.A, c.Lsh, c.C, c.Llg, K_, s, p, stream)
            assert rc == -1, 'the call after a failed one found the failed call\'s workspace'
        got = CC.run_wgrad(K, c, CC.EXACT, inp, 'cuda', call=call2)
        assert torch.equal(got['out'], inp['dw0']) and got['frame_ok'], 'a call that failed its argument check wrote dw'
        assert bool((ws == CC.SENTINEL).all())


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_conv_small_kernels(K, prec):
    seen, worst = [], {}
    with K.precision(prec):
        for ci, (label, c) in enumerate(CC.small_cases()):
            pl = CC.small_plan(c)
            rounded = prec == 'bf16' and c.op.startswith('o1')
            for pas in (CC.EXACT, CC.REAL):
                inp = CC.small_inputs(c, pas, 1000 + ci)
                ref = CC.small_reference(c, pas, inp, rounded)
                low = CC.small_reference(c, pas, inp, rounded, dtype=torch.float32)
                got = CC.run_small(K, c, pas, inp, 'cuda')
                again = CC.run_small(K, c, pas, inp, 'cuda') if pl['twostage'] else None
                assert set(got) == set(ref)
                for k in ref:
                    ratio = CC.check((label, c, k), pas, ref[k], got[k], floor=CC.floor_of(low[k], ref[k]), form=pl['kernel'], output=k,
                                     again=again[k] if again else None)
                    worst[pl['kernel'] + ':' + k] = max(worst.get(pl['kernel'] + ':' + k, 0.0), ratio)
            seen.append((label, c, pl))
    _report('small kernels', prec, worst)
    CC.assert_small_coverage(seen)
