"""-m gpu: the recurrent launches walked through their shape classes against float64 (tests/recurrent_cases.py) - the LSTM layer
(persistent forward in both clip tilings and at every H it accepts, persistent backward at its four H, the per-step kernels
with the fused and the skinny-product backward, the mixed pairing; fp32 mode and AG_PREC_BF16 teacher-forced step by step) and
the Generator fronts (LSTM and GRU cell, one launch and per frame, contiguous frames and channel 0 of a slab).

Every output sits NaN-filled between guard floats, every bound is margin * (the fp32 CPU model's own error against the same
float64 reference) and never above 1e-4 of the scale, the sticky status word of the persistent
launches is read after every case, and every case runs twice for bit-identical outputs.  Each test first asserts, with the
library's own ag_*_ok predicates and this device's CU count, that a case is of the class it stands for, counts the one-launch
wrappers to see that form really ran, and ends on the list of classes it must have met.  tests/test_recurrent_fuzz_host.py
shows on the CPU model that the checkers reject subtly wrong kernels."""
import collections

import pytest
import torch

from tests import recurrent_cases as RC

pytestmark = pytest.mark.gpu

LAYER_CALLS = ('_lstm_seq_fwd_persist_call', '_lstm_seq_bwd_persist_call')
FRONT_CALLS = ('gfront_fwd_persist', 'grufront_fwd_persist', 'gfront_bwd_persist', 'grufront_bwd_persist')


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    assert K_.lstm_seq_fwd.__module__ == 'audiogan_amd.kernels', 'real kernels must be in place'
    return K_


@pytest.fixture
def calls(K, monkeypatch):
    """counts the calls of the one-launch wrappers"""
    n = collections.Counter()
    for name in LAYER_CALLS + FRONT_CALLS:
        monkeypatch.setattr(K, name, lambda *a_, _o=getattr(K, name), _n=name, **k_: (n.update([_n]), _o(*a_, **k_))[1])
    return n


class persist_switch(object):
    def __init__(self, K, on):
        self.K, self.on = K, on

    def __enter__(self):
        self.old = self.K.PERSIST[0]
        self.K.PERSIST[0] = self.on

    def __exit__(self, *exc):
        self.K.PERSIST[0] = self.old


def _status_clean(K, what):
    """a non-zero sticky word fails the test at once: nothing further is launched, nothing is retried"""
    st = K.lstm_persist_status()
    assert st == 0, ('a persistent launch gave up', what, K.persist_error_text(st))


def _layer_class(K, case):
    """the class of a case as the LIBRARY sees it on this device: (forward persistent, its clip tiling, backward persistent).
    The tiling: a batch takes 64-clip tiles only where its grid of 32-clip tiles does not fit, and the 64-clip grid of 2 B
    clips is the 32-clip grid of B - so ag_lstm_persist_ok(2 B) says whether B runs on 32-clip tiles."""
    B, H, ndir = case['B'], case['H'], case['ndir']
    n_cu = K._n_cu(torch.device('cuda', torch.cuda.current_device()))
    fwd = bool(K.lib.ag_lstm_persist_ok(B, H, ndir, n_cu))
    rt = 0 if not fwd else 1 if K.lib.ag_lstm_persist_ok(2 * B, H, ndir, n_cu) else 2
    return fwd, rt, bool(K.lib.ag_lstm_persist_bwd_ok(B, H, ndir, n_cu))


def _assert_layer_class(K, case):
    fwd, rt, bwd = _layer_class(K, case)
    want = dict(fwd32=fwd and rt == 1, fwd64=fwd and rt == 2 and case['B'] % 64 != 0, bwd=bwd, step=not fwd and not bwd,
                mixed=fwd and not bwd)[case['cls']]
    assert want, ('this device does not run the case as its class says', case, fwd, rt, bwd)
    assert RC.layer_forms(case)[0] == ('fwd_persist<%d>' % rt if fwd else 'fwd_step')
    assert RC.layer_forms(case)[1].startswith('bwd_persist') == bwd
    return fwd, rt, bwd


def _report(title, worst):
    for form in sorted(worst):
        print('recurrent fuzz | %s | %-16s | %s' % (title, form, '  '.join('%s %.2f' % kv for kv in sorted(worst[form].items()))))


def _class_cases(cls):
    return [c for c in RC.layer_cases() if c['cls'] == cls]


@pytest.mark.parametrize('cls', list(RC.LAYER_CLASSES))
def test_layer_fp32_vs_float64(K, calls, cls):
    """forward + backward of every case of the class in fp32 mode; the persistent classes once more with K.PERSIST[0] = False
    (the same inputs and reference through the per-step kernels)"""
    dev = torch.device('cuda', torch.cuda.current_device())
    K.lstm_persist_status(reset=True)
    worst, met = {}, collections.Counter()
    with K.precision('f32'):
        for persist in ((True, False) if cls in RC.PERSISTENT_CLASSES else (True,)):
            for case in _class_cases(cls):
                fwd, rt, bwd = _assert_layer_class(K, case)
                inp, ref, floor = RC.prepared_layer(case)
                forms = RC.layer_forms(case, persist)
                with persist_switch(K, persist):
                    calls.clear()
                    got = RC.run_layer(K, case, inp, dev, options=persist)
                    _status_clean(K, case)
                    # the one-launch forms really ran where the class says so (and only there)
                    assert dict(calls) == {k: 1 for k, on in zip(LAYER_CALLS, (fwd, bwd)) if on and persist}, (case, dict(calls))
                    again = RC.run_layer(K, case, inp, dev, options=persist)
                    _status_clean(K, case)
                ratios = RC.check_layer(case, ref, floor, got, forms=forms, again=again)
                RC.merge_worst(worst, forms[0], {k: v for k, v in ratios.items() if k in ('y', 'c_all', 'gates')})
                RC.merge_worst(worst, forms[1], {k: v for k, v in ratios.items() if k in ('dgates', 'dgsum')})
                met.update([('kind', case['kind'], persist), ('forms', forms)])
                met.update(('opt', o, persist) for o in ('static', 'dgsum', 'y16', 'dy16', 'dg16') if case[o])
    _report('fp32 ' + cls, worst)
    for kind in RC.KINDS:               # every kind of lengths in every class, on both paths
        assert met[('kind', kind, True)] and (cls not in RC.PERSISTENT_CLASSES or met[('kind', kind, False)]), (cls, kind)
    forms_met = set(k[1] for k in met if k[0] == 'forms')
    need = dict(fwd32=[('fwd_persist<1>', None)], fwd64=[('fwd_persist<2>', None)],
                bwd=[(None, 'bwd_persist<%d>' % nu) for nu in (2, 4, 8, 16)],
                step=[('fwd_step', 'bwd_step'), ('fwd_step', 'bwd_skinny')], mixed=[('fwd_persist<1>', 'bwd_step')])[cls]
    for f, b in need:
        assert any((f is None or f == x) and (b is None or b == y) for x, y in forms_met), (cls, 'form never ran', f, b)
    if cls in RC.PERSISTENT_CLASSES:
        assert any(x == 'fwd_step' for x, _ in forms_met), (cls, 'never ran with the persistent launches off')
    if cls == 'fwd32':
        assert met[('opt', 'y16', True)], 'no bf16 y'
    if cls == 'bwd':
        assert met[('opt', 'dy16', True)] and met[('opt', 'dg16', True)] and met[('opt', 'dgsum', True)]


@pytest.mark.parametrize('cls', list(RC.LAYER_CLASSES))
def test_layer_bf16_mode_teacher_forced(K, calls, cls):
    """AG_PREC_BF16: every step of the forward, and at T = 2 both steps of the backward, recomputed in float64 from the GPU's
    own outputs of the step before with both operands of the recurrent product rounded to bf16; the unrounded step must be
    more than 10 times further away"""
    dev = torch.device('cuda', torch.cuda.current_device())
    K.lstm_persist_status(reset=True)
    worst, fwd_forms, bwd_forms = {}, set(), set()
    with K.precision('bf16'):
        for case in _class_cases(cls):
            fwd, rt, bwd = _assert_layer_class(K, case)
            inp, ref, _ = RC.prepared_layer(case)
            forms = RC.layer_forms(case)
            calls.clear()
            got = RC.run_layer(K, case, inp, dev, options=False)
            _status_clean(K, case)
            assert dict(calls) == {k: 1 for k, on in zip(LAYER_CALLS, (fwd, bwd)) if on}, (case, dict(calls))
            assert got['frames_ok'], ('guard frame: a store landed outside an output', case)
            again = RC.run_layer(K, case, inp, dev, options=False)
            _status_clean(K, case)
            for k in ('y', 'gates', 'c_all', 'dgates', 'dgsum'):
                assert RC.same_bits(got[k], again[k]), ('not reproducible: ' + k, case)
            T, B = case['T'], case['B']
            pad = (~ref['live']).view(T, B, 1)
            assert bool((got['y'][pad.expand_as(got['y'])] == 0).all()), ('padded y is not 0', case)
            for dg in got['dgates']:
                assert bool((dg[pad.expand_as(dg)] == 0).all()), ('padded dgates is not 0', case)
            ratios = RC.check_tf(case, inp, got, ref['live'], forms)
            RC.merge_worst(worst, forms[0], {k: v for k, v in ratios.items() if not k.startswith('dgates')})
            RC.merge_worst(worst, forms[1], {k: v for k, v in ratios.items() if k.startswith('dgates')})
            if fwd and T > 1:
                # the bf16 forward form is a function of (tiling, parity of H / 64): 32-clip tiles hold H / 64 unit tiles per
                # wave - even: the bf16 MFMA <RT,2>, odd: operands rounded in front of the fp32 MFMA <RT,1>
                fwd_forms.add((rt, 'even' if (case['H'] // 64) % 2 == 0 or rt == 2 else 'odd'))
            if T == 2:
                bwd_forms.add(forms[1])
    _report('bf16 ' + cls, worst)
    # <2,1> cannot occur: with 64-clip tiles the per-wave tile count is H / 32, which is always even
    need = dict(fwd32={(1, 'odd'), (1, 'even')}, fwd64={(2, 'even')}, mixed={(1, 'odd')}).get(cls, set())
    assert need <= fwd_forms, (cls, 'bf16 forward form never ran', need - fwd_forms)
    need_b = dict(bwd={'bwd_persist<%d>' % nu for nu in (2, 4, 8, 16)}, step={'bwd_step', 'bwd_skinny'}, mixed={'bwd_step'}).get(cls, set())
    assert need_b <= bwd_forms, (cls, 'bf16 backward form never checked at T = 2', need_b - bwd_forms)


# ---------------------------------------------------------------------------------------------------------------------
# fronts
# ---------------------------------------------------------------------------------------------------------------------
def _run_front(K, monkeypatch, cell, case, inp, slab):
    """forward + backward of one front through its autograd block, the frames written into a NaN-filled [B, ctot, T * fs]
    buffer between guard floats (ctot = 3: channel 0 of a slab, the gradient handed back as a row-pitched view)"""
    from audiogan_amd import ops, recurrent
    S, fs, B, T = case['S'], case['fs'], case['B'], case['T']
    front = ops.GRUFront(fs, S) if cell == 'gru' else ops.GFront(fs, 1, S)
    for v, g in inp['vg']:
        front.group.add(torch.nn.Parameter(v.cuda()), torch.nn.Parameter(g.cuda().clone()))
    params = list(front.group.params())
    zc = inp['zc'].cuda().requires_grad_(True)
    ctot = 3 if slab else 1
    fr = RC.Framed((B, ctot, T * fs), 'cuda')

    def into_frame(front_, B_, n, dev):
        assert (B_, n) == (B, T * fs)
        return fr.t[:, 0, :]
    monkeypatch.setattr(recurrent, '_frames_buffer', into_frame)
    fn = ops.GRUFrontFn if cell == 'gru' else ops.GFrontFn
    x, s = fn.apply(zc, front, *params)
    assert x.data_ptr() == fr.t.data_ptr() and x.stride(0) == ctot * T * fs
    gx, gs = inp['gx'].cuda(), inp['gs'].cuda()
    if slab:
        gx_wide = torch.zeros(B, 3, T * fs, device='cuda')
        gx_wide[:, 0] = gx
        x.backward(gx_wide[:, 0], retain_graph=True)
        (s * gs).sum().backward()
    else:
        ((x * gx).sum() + (s * gs).sum()).backward()
    torch.cuda.synchronize()
    ok = fr.intact() and bool(torch.isnan(fr.t[:, 1:]).all())
    if slab:
        ok = ok and not bool(gx_wide[:, 1:].any()) and torch.equal(gx_wide[:, 0], gx)
    cpu = lambda t: t.detach().cpu().clone()      # noqa: E731
    return dict(x=cpu(x), s=cpu(s), dzc=cpu(zc.grad), grads=[cpu(q.grad) for q in params], frames_ok=ok)


@pytest.mark.parametrize('cell', ['lstm', 'gru'])
def test_front_vs_float64(K, calls, monkeypatch, cell):
    """frames, stop logits, dzc and the gradient of every v and g of the WNGroup against ref_front's autograd, the one-launch
    form and the per-frame path EACH against float64, contiguous frames and channel 0 of a slab"""
    from audiogan_amd import recurrent
    dev = torch.device('cuda', torch.cuda.current_device())
    n_cu = K._n_cu(dev)
    K.lstm_persist_status(reset=True)
    plain = recurrent._frames_buffer
    worst, met = {}, set()
    names = ('grufront_fwd_persist', 'grufront_bwd_persist') if cell == 'gru' else ('gfront_fwd_persist', 'gfront_bwd_persist')
    try:
        with K.precision('f32'):
            for case in RC.front_cases():
                S, fs, B = case['S'], case['fs'], case['B']
                assert K.lib.ag_gfront_persist_ok(B, S, fs, n_cu) and K.lib.ag_gfront_bwd_persist_ok(B, S, fs, n_cu), case
                inp, ref, floor = RC.prepared_front(case, cell)
                for persist in (True, False):
                    form = 'front_%s_%s' % (cell, 'persist' if persist else 'frames')
                    for slab in (False, True):
                        with persist_switch(K, persist):
                            calls.clear()
                            got = _run_front(K, monkeypatch, cell, case, inp, slab)
                            _status_clean(K, case)
                            # (the slab pass calls backward twice, once per output: two backward launches)
                            want = {names[0]: 1, names[1]: 2 if slab else 1} if persist else {}
                            assert dict(calls) == want, (case, persist, slab, dict(calls))
                            again = _run_front(K, monkeypatch, cell, case, inp, slab)
                            _status_clean(K, case)
                        RC.merge_worst(worst, form, RC.check_front(case, inp, ref, floor, got, form=form, again=again))
                        met.add((case['cls'], persist, slab))
    finally:
        monkeypatch.setattr(recurrent, '_frames_buffer', plain)
    _report('fronts', worst)
    assert met == {(c, p, s) for c in RC.FRONT_CLASSES for p in (True, False) for s in (True, False)}
    RC.assert_front_classes(RC.front_cases())


def test_layer_table_holds_every_required_class():
    RC.assert_layer_classes(RC.layer_cases())
