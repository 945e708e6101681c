"""-m gpu: the stacked front's backward through time in ONE persistent launch (ag_gfront_stack_bwd, 2 to 8 layers) - every case
of tests/stacked_front_bwd_cases.py end to end against float64 through recurrent.GFrontFn (forward and backward one launch
each), the direct launch against the float64 chain on the saved history with the per-frame path's own error as the floor,
bf16 mode, the module level inside one captured graph and with K.front_bwd_persist(False), and the profiler's name.  The
sticky status word of the persistent launches is read after every run.  tests/test_front_stack_bwd.py shows on a CPU model that
the checkers reject subtly wrong launches."""
import collections

import pytest
import torch

from oracle import audiogan_oracle as O
from tests import stacked_front_bwd_cases as BC
from tests import stacked_front_cases as SC

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    assert K_.gfront_stack_bwd_persist.__module__ == 'audiogan_amd.kernels', 'real kernels must be in place'
    assert K_.PERSIST[0] and K_.PERSIST_FRONT_STACK[0] and K_.PERSIST_FRONT_BWD[0]
    return K_


@pytest.fixture
def on(K):
    """the tests run the launch whatever the shipped default of its switch is"""
    old = K.PERSIST_FRONT_STACK_BWD[0]
    K.PERSIST_FRONT_STACK_BWD[0] = True
    yield
    K.PERSIST_FRONT_STACK_BWD[0] = old


@pytest.fixture
def calls(K, monkeypatch):
    """counts the calls of the stacked launches' wrappers and of the per-frame cell backward"""
    n = collections.Counter()
    for name, tag in (('gfront_stack_fwd_persist', 'fwd'), ('gfront_stack_bwd_persist', 'bwd'), ('lstm_cell_bwd', 'cell_bwd')):
        monkeypatch.setattr(K, name, lambda *a_, _o=getattr(K, name), _n=tag, **k_: (n.update([_n]), _o(*a_, **k_))[1])
    return n


class bwd_switch(object):
    def __init__(self, K, on):
        self.K, self.on = K, on

    def __enter__(self):
        self.old = self.K.PERSIST_FRONT_STACK_BWD[0]
        self.K.PERSIST_FRONT_STACK_BWD[0] = self.on

    def __exit__(self, *exc):
        self.K.PERSIST_FRONT_STACK_BWD[0] = self.old


def _status_clean(K, what):
    """a non-zero sticky word fails the test at once: nothing further is launched, nothing is retried"""
    torch.cuda.synchronize()
    st = K.lstm_persist_status()
    assert st == 0, ('a persistent launch gave up', what, K.persist_error_text(st))


def _assert_class(K, nl, S, fs, B):
    n_cu = K._n_cu(torch.device('cuda', torch.cuda.current_device()))
    assert K.lib.ag_gfront_stack_bwd_ok(B, S, fs, nl, n_cu) == 1, ('this device does not run the case as one launch', nl, S, fs, B, n_cu)
    assert K.gfront_stack_bwd_ok(B, S, fs, nl, torch.device(DEV))


# ---------------------------------------------------------------------------------------------------------------------
# (a) every case end to end against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', BC.BWD_CASES, ids=SC.case_name)
def test_case_vs_float64(K, on, calls, monkeypatch, case):
    """frames, stop logits, dzc and the gradient of every v and g against ref_stack_front's autograd; contiguous frames and
    channel 0 of a NaN-filled slab, each run twice for identical bits; forward and backward one launch each (the slab form
    runs two backward passes: frames, then stop logits), no per-frame cell backward"""
    _assert_class(K, case['nl'], case['S'], case['fs'], case['B'])
    fwd = 1 if K.lib.ag_gfront_stack_ok(case['B'], case['S'], case['fs'], case['nl'], K._n_cu(torch.device('cuda', 0))) else 0
    K.lstm_persist_status(reset=True)
    inp, ref, floor = SC.prepared_stack(case)
    with K.precision('f32'):
        for slab in (False, True):
            calls.clear()
            got = SC.run_stack_front(monkeypatch, case, inp, DEV, slab)
            _status_clean(K, case)
            want = {'bwd': 2 if slab else 1}
            if fwd:
                want['fwd'] = 1
            assert dict(calls) == want, dict(calls)
            again = SC.run_stack_front(monkeypatch, case, inp, DEV, slab)
            _status_clean(K, case)
            ratios = SC.check_stack(case, inp, ref, floor, got, again=again)
            worst = max(ratios, key=ratios.get)
            print('stacked front bwd ratio | %s | %s | x %.2f  s %.2f  dzc %.2f  worst %s %.2f' % (
                SC.case_name(case), 'slab' if slab else 'contiguous', ratios['x'], ratios['s'], ratios['dzc'], worst, ratios[worst]))


# ---------------------------------------------------------------------------------------------------------------------
# (b) the direct launch against the chain, the per-frame path as the floor
# ---------------------------------------------------------------------------------------------------------------------
def _history_and_per_frame(K, monkeypatch, case, inp):
    """one forward; its backward with the switch off: returns (the launch's arguments on that saved history, the per-frame
    path's dgs / dxt)"""
    from audiogan_amd import ops, recurrent
    nl, S, fs, B, T = case['nl'], case['S'], case['fs'], case['B'], case['T']
    front = SC.build_front(case, inp, DEV)
    seen = []
    orig = recurrent.GFrontFn._bwd_frames

    def spy(T_, B_, fs_, S_, nl_, x, dx, ds, gates, cs, lw, wx, pw, sw, hs, dws):
        dgs, dxt = orig(T_, B_, fs_, S_, nl_, x, dx, ds, gates, cs, lw, wx, pw, sw, hs, dws)
        ds_tb = recurrent._stop_head_grads(ds, hs[-1].view(T * B, S), None, 4 * nl + 2)
        dh_ext, dx_ext = recurrent._ext_grads(ds_tb, sw, dx, T, B, S)
        seen.append((dict(gates=list(gates), cs=list(cs), x=x, dh_ext=dh_ext, dx_ext=dx_ext, whh=[lw[l][1] for l in range(nl)],
                          w_in=[lw[l][0] for l in range(1, nl)], wx=wx, wp=pw),
                     dict(dgs=[d.detach().cpu().clone() for d in dgs], dxt=dxt.detach().cpu().clone(), frames_ok=True)))
        return dgs, dxt
    monkeypatch.setattr(recurrent.GFrontFn, '_bwd_frames', staticmethod(spy))
    try:
        with bwd_switch(K, False):
            x, s = ops.GFrontFn.apply(inp['zc'].to(DEV).clone().requires_grad_(True), front, *front.group.params())
            ((x * inp['gx'].to(DEV)).sum() + (s * inp['gs'].to(DEV)).sum()).backward()
    finally:
        monkeypatch.setattr(recurrent.GFrontFn, '_bwd_frames', staticmethod(orig))
    (h, per_frame), = seen
    return h, per_frame


@pytest.mark.parametrize('case', BC.BWD_CASES, ids=SC.case_name)
def test_direct_launch_vs_chain(K, on, monkeypatch, case):
    """ONE forward's saved history feeds the launch and the per-frame chain (the parent's code), the same dx / ds: every dgs[l]
    and dxt NaN-filled between guard floats, against stack_bwd_chain in float64 on that history; bound = 16 x the per-frame
    path's own error against the chain (never below 16 x 2^-24, never above 1e-4 of the tensor's largest magnitude)"""
    _assert_class(K, case['nl'], case['S'], case['fs'], case['B'])
    K.lstm_persist_status(reset=True)
    inp, _, _ = SC.prepared_stack(case)
    with K.precision('f32'):
        h, per_frame = _history_and_per_frame(K, monkeypatch, case, inp)
        got = BC.run_direct(K.gfront_stack_bwd_persist, h, DEV)
        _status_clean(K, case)
        again = BC.run_direct(K.gfront_stack_bwd_persist, h, DEV)
        _status_clean(K, case)
    chain = BC.stack_bwd_chain(h['gates'], h['cs'], h['x'], h['dh_ext'], h['dx_ext'], h['whh'], h['w_in'], h['wx'], h['wp'])
    floor = BC.direct_errors(chain, per_frame)
    ratios = BC.check_direct(SC.case_name(case), chain, floor, got, again=again)
    print('stacked front bwd direct | %s | %s' % (SC.case_name(case), '  '.join('%s %.2f' % kv for kv in sorted(ratios.items()))))


# ---------------------------------------------------------------------------------------------------------------------
# (c) bf16 mode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [BC.BWD_CASES[0], BC.BWD_CASES[7]], ids=SC.case_name)
def test_bf16_mode(K, on, calls, monkeypatch, case):
    """AG_PREC_BF16 (both operands of all four products rounded in registers in front of the fp32 MFMA): the launch against the
    per-frame path in bf16 mode, at the tolerance of the bf16 front tests"""
    from tests.test_bf16 import close_bf16
    _assert_class(K, case['nl'], case['S'], case['fs'], case['B'])
    K.lstm_persist_status(reset=True)
    inp, _, _ = SC.prepared_stack(case)
    old = K.set_precision('bf16')
    try:
        calls.clear()
        got = SC.run_stack_front(monkeypatch, case, inp, DEV)
        assert calls['bwd'] == 1 and calls['cell_bwd'] == 0, dict(calls)
        with bwd_switch(K, False):
            ref = SC.run_stack_front(monkeypatch, case, inp, DEV)
        assert calls['bwd'] == 1 and calls['cell_bwd'] == case['nl'] * case['T'], dict(calls)
    finally:
        K.set_precision(old)
    _status_clean(K, case)
    close_bf16(got['dzc'], ref['dzc'], 'dzc')
    names = [n + s_ for n in SC.param_names(case['nl']) for s_ in ('_v', '_g')]
    for i, name in enumerate(names):
        a, b = got['grads'][i], ref['grads'][i]
        if name.endswith('_v') and '.b' in name:
            # the v-gradient of a bias is analytically zero (w = g v / |v| of a one-element row does not depend on |v|): both
            # sides hold fp32 rounding noise of the size 1e-7 of dg, which no relative tolerance describes
            assert float(a.abs().max()) <= 1e-5 * max(float(got['grads'][i + 1].abs().max()), 1e-6), name
            continue
        close_bf16(a, b, name)


# ---------------------------------------------------------------------------------------------------------------------
# (d) module level
# ---------------------------------------------------------------------------------------------------------------------
GCFG = dict(frame_size=64, embed_size=8, noise_size=8, state_size=128, num_layers=2, struct=[[17, 8, 16, 8], [9, 4, 16, 8]])


def _pair():
    import audiogan_amd as A
    torch.manual_seed(11)
    go = O.Generator(**GCFG)
    g = A.Generator(**GCFG)
    g.load_state_dict(go.state_dict())
    return g.cuda(), go


def test_generator_vs_oracle_and_the_multi_gpu_switch(K, on, calls):
    """every parameter gradient of a two-layer Generator against the oracle at the tolerances of tests/test_gpu_modules.py, by
    the one launch and, under K.front_bwd_persist(False), by the per-frame chain"""
    from tests.test_gpu_modules import _grads_close, close as mclose
    B, T = 5, 6
    gen = torch.Generator().manual_seed(1)
    z, c = torch.randn(B, T, 8, generator=gen), torch.randn(B, 8, generator=gen)
    wx, ws = torch.randn(B, T * 64, generator=gen), torch.randn(B, T, generator=gen)
    K.lstm_persist_status(reset=True)
    for persist in (True, False):
        g, go = _pair()
        assert K.gfront_stack_bwd_ok(B, 128, 64, 2, torch.device(DEV))
        xo, so, _, lo = go(z=z, c=c, stop=torch.zeros(B, T, dtype=torch.long))
        ((xo * wx).sum() + (so * ws).sum()).backward()
        calls.clear()
        x, s, _, ln = g(z=z.cuda(), c=c.cuda(), stop='never')
        with K.front_bwd_persist(persist):
            ((x * wx.cuda()).sum() + (s * ws.cuda()).sum()).backward()
        _status_clean(K, 'generator')
        assert dict(calls) == ({'fwd': 1, 'bwd': 1} if persist else {'fwd': 1, 'cell_bwd': 2 * T}), dict(calls)
        mclose(x, xo); mclose(s, so)
        _grads_close(g, {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in go.named_parameters()})


def test_generator_forward_and_backward_in_one_graph(K, on, calls):
    """forward (stop='never') + backward captured into ONE torch.cuda.graph: two replays equal the eager gradients bit for bit.
    The eager reference step runs on the capturing stream (as the forward's graph test does), after the side-stream warm-up that
    autograd capture asks for.  Finding, not explained yet: with the side-stream warm-up ALONE before the capture the first replay
    equals eager and the second differs in the front's gradients (up to 4e-2 of a bias gradient), with this launch and, in the
    same set-up, with the one-layer launch ag_gfront_bwd that this change does not touch; the per-frame chain replays equal."""
    from tests.test_gpu_generate import _inputs
    g, _ = _pair()
    B, T = 33, 4
    assert K.gfront_stack_bwd_ok(B, 128, 64, 2, torch.device(DEV))
    K.lstm_persist_status(reset=True)
    z, c = _inputs(B, T, 8, 8, 7)
    gen = torch.Generator().manual_seed(5)
    wx, ws = torch.randn(B, T * 64, generator=gen).cuda(), torch.randn(B, T, generator=gen).cuda()
    params = list(g.parameters())

    def step():
        for p in params:
            p.grad = None
        x, s, _, _ = g(z=z, c=c, stop='never')
        ((x * wx).sum() + (s * ws).sum()).backward()

    K.reserve_table_arena()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                          # warm-up (also: workspaces and weight caches exist before capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    step()                                              # the eager reference, on the stream the capture will use
    torch.cuda.synchronize()
    eager = [p.grad.clone() for p in params]
    graph = torch.cuda.CUDAGraph()
    calls.clear()
    with torch.cuda.graph(graph):
        step()
    assert dict(calls) == {'fwd': 1, 'bwd': 1}, dict(calls)
    grads = [p.grad for p in params]
    for _ in range(2):
        for q in grads:
            q.zero_()                                   # (a replay that wrote nothing would leave zeros)
        graph.replay()
        torch.cuda.synchronize()
        bad = [(n, float((q - e).abs().max())) for (n, _), q, e in zip(g.named_parameters(), grads, eager) if not torch.equal(q, e)]
        assert not bad, ('replay differs from eager', len(bad), bad[:8])
    _status_clean(K, 'graph')


# ---------------------------------------------------------------------------------------------------------------------
# (e) profiler
# ---------------------------------------------------------------------------------------------------------------------
def test_profiler_files_the_launch_under_its_kernel_name(K, on, monkeypatch):
    """under K.Profiler the launch is filed exactly once, under the name its launch site reported"""
    case = BC.BWD_CASES[0]
    inp, _, _ = SC.prepared_stack(case)
    K.lstm_persist_status(reset=True)
    with K.precision('f32'):
        K.Profiler.start()
        try:
            SC.run_stack_front(monkeypatch, case, inp, DEV)
        finally:
            prof = K.Profiler.stop()
    names = [k for k in prof if 'front_stack_bwd' in k]
    assert names == ['gfront_stack_bwd_kernel<128,64,0>'] and prof[names[0]]['n'] == 1, prof
    _status_clean(K, 'profiler')
