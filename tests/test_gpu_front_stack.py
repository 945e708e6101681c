"""-m gpu: stacked LSTM fronts in ONE persistent launch (ag_gfront_stack_fwd, 2 to 8 layers), training forward and generation
mode - every case of tests/stacked_front_cases.py against float64 through recurrent.GFrontFn (forward by the new launch,
backward by the unchanged per-frame chain), the history the launch writes against the per-frame path, the generation mode
against the training launch and against Generator.forward given the same stop draws, bf16 mode, the module level against the
oracle and inside one captured graph, and the profiler's name.  Bounds: the rule of tests/recurrent_cases.py (margin * the
fp32 model's own error against the same float64 reference, never above 1e-4 of the scale); the sticky status word of the
persistent launches is read after every case.  tests/test_front_stack.py shows on a CPU model that the checkers reject
subtly wrong launches."""
import collections

import pytest
import torch

from oracle import audiogan_oracle as O
from tests import stacked_front_cases as SC
from tests.test_gpu_generate import GEN_LAG, _inputs, _pattern, close

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    assert K_.gfront_stack_fwd_persist.__module__ == 'audiogan_amd.kernels', 'real kernels must be in place'
    assert K_.PERSIST[0] and K_.PERSIST_FRONT_STACK[0]
    return K_


@pytest.fixture
def calls(K, monkeypatch):
    """counts the calls of the stacked launch's two wrappers"""
    n = collections.Counter()
    for name in ('gfront_stack_fwd_persist', 'gfront_stack_gen_persist'):
        monkeypatch.setattr(K, name, lambda *a_, _o=getattr(K, name), _n=name, **k_: (n.update([_n]), _o(*a_, **k_))[1])
    return n


class stack_switch(object):
    def __init__(self, K, on):
        self.K, self.on = K, on

    def __enter__(self):
        self.old = self.K.PERSIST_FRONT_STACK[0]
        self.K.PERSIST_FRONT_STACK[0] = self.on

    def __exit__(self, *exc):
        self.K.PERSIST_FRONT_STACK[0] = self.old


def _status_clean(K, what):
    """a non-zero sticky word fails the test at once: nothing further is launched, nothing is retried"""
    torch.cuda.synchronize()
    st = K.lstm_persist_status()
    assert st == 0, ('a persistent launch gave up', what, K.persist_error_text(st))


def _assert_class(K, nl, S, fs, B):
    n_cu = K._n_cu(torch.device('cuda', torch.cuda.current_device()))
    assert K.lib.ag_gfront_stack_ok(B, S, fs, nl, n_cu) == 1, ('this device does not run the case as one launch', nl, S, fs, B, n_cu)
    assert K.gfront_stack_ok(B, S, fs, nl, torch.device(DEV))


# ---------------------------------------------------------------------------------------------------------------------
# every case against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', SC.CASES, ids=SC.case_name)
def test_case_vs_float64(K, calls, monkeypatch, case):
    """frames, stop logits, dzc and the gradient of every v and g against ref_stack_front's autograd; contiguous frames and
    channel 0 of a NaN-filled slab, each run twice for identical bits"""
    _assert_class(K, case['nl'], case['S'], case['fs'], case['B'])
    K.lstm_persist_status(reset=True)
    inp, ref, floor = SC.prepared_stack(case)
    with K.precision('f32'):
        for slab in (False, True):
            calls.clear()
            got = SC.run_stack_front(monkeypatch, case, inp, DEV, slab)
            _status_clean(K, case)
            assert dict(calls) == {'gfront_stack_fwd_persist': 1}, dict(calls)
            again = SC.run_stack_front(monkeypatch, case, inp, DEV, slab)
            _status_clean(K, case)
            ratios = SC.check_stack(case, inp, ref, floor, got, again=again)
            worst = max(ratios, key=ratios.get)
            print('stacked front ratio | %s | %s | x %.2f  s %.2f  dzc %.2f  worst %s %.2f' % (
                SC.case_name(case), 'slab' if slab else 'contiguous', ratios['x'], ratios['s'], ratios['dzc'], worst, ratios[worst]))


# ---------------------------------------------------------------------------------------------------------------------
# the history the launch writes
# ---------------------------------------------------------------------------------------------------------------------
def _weights(front, nl, fs):
    prep = front.group.prepare()
    lw = [[p.w for p in prep[4 * l:4 * l + 4]] for l in range(nl)]
    return lw, [p.w for p in prep[4 * nl:4 * nl + 4]]


@pytest.mark.parametrize('case', SC.CASES, ids=SC.case_name)
def test_history_equals_the_per_frame_path(K, monkeypatch, case):
    """gates[l], hs[l], cs[l], xt and x of ONE direct launch, every output NaN-filled between guard floats, against what the
    per-frame path (switch off) hands its backward; cs[l][0] == 0 is written by the launch"""
    from audiogan_amd import ops, recurrent
    nl, S, fs, B, T = case['nl'], case['S'], case['fs'], case['B'], case['T']
    _assert_class(K, nl, S, fs, B)
    K.lstm_persist_status(reset=True)
    inp, _, _ = SC.prepared_stack(case)
    front = SC.build_front(case, inp, DEV)
    zc = inp['zc'].to(DEV)
    seen = []
    orig = recurrent.GFrontFn._bwd_frames

    def spy(T_, B_, fs_, S_, nl_, x, dx, ds, gates, cs, lw, wx, pw, sw, hs, dws):
        seen.append(dict(gates=[g.clone() for g in gates], hs=[h.clone() for h in hs], cs=[c.clone() for c in cs], x=x.clone()))
        return orig(T_, B_, fs_, S_, nl_, x, dx, ds, gates, cs, lw, wx, pw, sw, hs, dws)
    monkeypatch.setattr(recurrent.GFrontFn, '_bwd_frames', staticmethod(spy))
    with K.precision('f32'):
        with stack_switch(K, False):
            x0, s0 = ops.GFrontFn.apply(zc.clone().requires_grad_(True), front, *front.group.params())
            (x0.sum() + s0.sum()).backward()
        (ref,) = seen
        lw, (pw, pb, sw, sb) = _weights(front, nl, fs)
        wx, wz = lw[0][0][:, :fs], lw[0][0][:, fs:]
        F = lambda *shape: SC.Framed(shape, DEV)      # noqa: E731
        gates, hs, cs = [F(T, B, 4 * S) for _ in range(nl)], [F(T, B, S) for _ in range(nl)], [F(T + 1, B, S) for _ in range(nl)]
        x, xt = F(B, T * fs), F(T, B, fs)
        recurrent._front_pre(zc, wz, lw[0][2], lw[0][3], gates[0].t, gru=False)
        K.gfront_stack_fwd_persist([g.t for g in gates], wx, [lw[l][0] for l in range(1, nl)], [lw[l][1] for l in range(nl)],
                                   [lw[l][2] + lw[l][3] for l in range(1, nl)], pw, pb, [h.t for h in hs], [c.t for c in cs], x.t, xt.t)
    _status_clean(K, case)
    for name, bufs in (('gates', gates), ('hs', hs), ('cs', cs)):
        for l in range(nl):
            assert bufs[l].intact(), ('guard frame', name, l)
            close(bufs[l].t, ref[name][l], rtol=1e-4, msg='%s[%d]' % (name, l))
    assert x.intact() and xt.intact()
    close(x.t, ref['x'], rtol=1e-4, msg='x')
    assert torch.equal(xt.t.permute(1, 0, 2).reshape(B, T * fs), x.t), 'xt is x time-major'
    for l in range(nl):
        assert not bool(cs[l].t[0].any()) and not bool(torch.isnan(cs[l].t).any()), ('cs[%d][0]' % l)


# ---------------------------------------------------------------------------------------------------------------------
# generation mode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nl,S,fs,B,T', [(2, 128, 64, 7, 1), (2, 128, 64, 40, 6), (2, 1024, 256, 32, 4), (3, 128, 24, 33, 3)])
def test_generation_launch_matches_training_launch(K, calls, nl, S, fs, B, T):
    """u = 1 (no clip ever stops): frames and stop logits are those of the training launch over all T frames; every frame runs
    and first = T"""
    from audiogan_amd import ops
    from audiogan_amd.recurrent import front_sample
    _assert_class(K, nl, S, fs, B)
    K.lstm_persist_status(reset=True)
    case = dict(id=200 + nl + B, nl=nl, S=S, fs=fs, B=B, T=T)
    inp = SC.make_stack_inputs(case)
    front = SC.build_front(case, inp, DEV)
    zc = inp['zc'].to(DEV)
    with torch.no_grad(), K.precision('f32'):
        x_ref, s_ref = ops.GFrontFn.apply(zc, front, *front.group.params())
        x, s, first, t_run = front_sample(front, zc, torch.ones(T, B, device=DEV))
    _status_clean(K, case)
    assert dict(calls) == {'gfront_stack_fwd_persist': 1, 'gfront_stack_gen_persist': 1}, dict(calls)
    close(x, x_ref, rtol=1e-4, atol=1e-6, msg='frames')
    close(s, s_ref, rtol=1e-4, msg='stop logits')
    assert int(t_run) == T and first.dtype == torch.int64 and bool((first == T).all())


def _generator(S, fs):
    import audiogan_amd as A
    torch.manual_seed(41)
    if S == 1024:
        cfg = dict(frame_size=fs, embed_size=100, noise_size=100, state_size=S)
    else:
        cfg = dict(frame_size=fs, embed_size=8, noise_size=8, state_size=S, struct=[[17, 8, 16, 8], [9, 4, 16, 8]])
    return A.Generator(num_layers=2, **cfg).cuda(), cfg['noise_size'], cfg['embed_size']


def _early_exit(K, calls, S, fs, B, on, tol=None, ref_on=None):
    """generate with the last stop at frame 5 of 32 (switch `on`) against Generator.forward given the same draws (switch
    `ref_on`, default the same)"""
    T = 32
    g, ns, es = _generator(S, fs)
    z, c = _inputs(B, T, ns, es, 43)
    u, stops, frames = _pattern(B, T)
    K.lstm_persist_status(reset=True)
    calls.clear()
    with stack_switch(K, on):
        wave, s, stop_list, length = g.generate(c, z=z, u=u)
    t_run = g.last_t_run
    with torch.no_grad(), stack_switch(K, on if ref_on is None else ref_on):
        wf, sf, _, lf = g(z=z, c=c, stop=stops)
    _status_clean(K, (S, fs, B, on))
    assert torch.equal(length, (frames + 1) * fs) and torch.equal(lf, length)          # `first` exact
    if on:
        assert calls['gfront_stack_gen_persist'] == 1
        assert 6 <= int(t_run) <= 6 + GEN_LAG, int(t_run)
    else:
        assert calls['gfront_stack_gen_persist'] == 0 and t_run is None
    assert len(stop_list) == 6 and torch.equal(torch.cat(stop_list, 1), stops[:, :6])
    if tol is None:
        close(wave, wf, rtol=1e-4, msg='wave')
        close(s, sf, rtol=1e-4, msg='stop logits')
    else:
        tol(wave, wf, 'wave')
        tol(s, sf, 'stop logits')


@pytest.mark.parametrize('on', [True, False])
@pytest.mark.parametrize('S,fs,B', [(128, 64, 1), (128, 64, 33), (128, 64, 64), (1024, 256, 32)])
def test_generate_exits_early_and_matches_forward(K, calls, S, fs, B, on):
    """stops drawn at known frames: first is exact, the loop ran at most 6 + GEN_LAG frames, stop_list / length / wave / logits
    are Generator.forward's given the same draws; the same with the switch off, where last_t_run is None"""
    _assert_class(K, 2, S, fs, B)
    _early_exit(K, calls, S, fs, B, on)


def test_generate_bf16_mode(K, calls):
    """AG_PREC_BF16 (operands rounded in registers in front of the fp32 MFMA): the early-exit case against the per-frame path in
    bf16 mode, at the tolerance of the bf16 front tests"""
    from tests.test_bf16 import close_bf16
    old = K.set_precision('bf16')
    try:
        _early_exit(K, calls, 128, 64, 33, True, tol=lambda a, b, m: close_bf16(a, b, m), ref_on=False)
    finally:
        K.set_precision(old)


# ---------------------------------------------------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------------------------------------------------
GCFG = dict(frame_size=64, embed_size=8, noise_size=8, state_size=128, num_layers=2, struct=[[17, 8, 16, 8], [9, 4, 16, 8]])


def _pair():
    import audiogan_amd as A
    torch.manual_seed(11)
    go = O.Generator(**GCFG)
    g = A.Generator(**GCFG)
    g.load_state_dict(go.state_dict())
    return g.cuda(), go


def test_generator_vs_oracle(K, calls):
    """forward and every parameter gradient of a two-layer Generator against the oracle, at the tolerances of
    tests/test_gpu_modules.py; the front ran as the one launch"""
    from tests.test_gpu_modules import _grads_close, close as mclose
    g, go = _pair()
    B, T = 5, 6
    assert g.front_is_persistent(B, torch.device(DEV)) is True
    K.lstm_persist_status(reset=True)
    gen = torch.Generator().manual_seed(1)
    z, c = torch.randn(B, T, 8, generator=gen), torch.randn(B, 8, generator=gen)
    wx, ws = torch.randn(B, T * 64, generator=gen), torch.randn(B, T, generator=gen)
    xo, so, _, lo = go(z=z, c=c, stop=torch.zeros(B, T, dtype=torch.long))
    ((xo * wx).sum() + (so * ws).sum()).backward()
    x, s, _, ln = g(z=z.cuda(), c=c.cuda(), stop='never')
    ((x * wx.cuda()).sum() + (s * ws.cuda()).sum()).backward()
    _status_clean(K, 'generator')
    assert dict(calls) == {'gfront_stack_fwd_persist': 1}, dict(calls)
    mclose(x, xo); mclose(s, so)
    assert torch.equal(ln.cpu(), lo)
    _grads_close(g, {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in go.named_parameters()})


def test_generator_forward_in_one_graph(K, calls):
    """the forward (stop='never') captured into ONE torch.cuda.graph on a single stream: two replays equal the eager result
    bit for bit"""
    g, _ = _pair()
    B, T = 33, 4
    assert g.front_is_persistent(B, torch.device(DEV)) is True
    K.lstm_persist_status(reset=True)
    z, c = _inputs(B, T, 8, 8, 7)
    with torch.no_grad():
        x0, s0, _, _ = g(z=z, c=c, stop='never')          # eager (also: workspaces and weight caches exist before capture)
        x0, s0 = x0.clone(), s0.clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        calls.clear()
        with torch.cuda.graph(graph):
            x1, s1, _, _ = g(z=z, c=c, stop='never')
        assert dict(calls) == {'gfront_stack_fwd_persist': 1}, dict(calls)
        for _ in range(2):
            x1.zero_(); s1.zero_()                          # (a replay that wrote nothing would leave zeros)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(x1, x0) and torch.equal(s1, s0)
    _status_clean(K, 'graph')


def test_profiler_files_the_launch_under_its_kernel_name(K):
    """under K.Profiler the launch is filed exactly once, under the name its launch site reported"""
    from audiogan_amd import ops
    case = SC.CASES[0]
    inp, _, _ = SC.prepared_stack(case)
    front = SC.build_front(case, inp, DEV)
    zc = inp['zc'].to(DEV)
    K.lstm_persist_status(reset=True)
    with torch.no_grad(), K.precision('f32'):
        K.Profiler.start()
        try:
            ops.GFrontFn.apply(zc, front, *front.group.params())
        finally:
            prof = K.Profiler.stop()
    names = [k for k in prof if 'front' in k]
    assert len(names) == 1 and names[0].startswith('gfront_stack_fwd_kernel<') and prof[names[0]]['n'] == 1, prof
    assert names == ['gfront_stack_fwd_kernel<128,64,0>'], names
    _status_clean(K, 'profiler')
