"""The conv dispatch fuzz (tests/conv_cases.py) against the CPU model of the kernels: the case lists, plans, runners,
references and checker that tests/test_conv_fuzz.py turns on the HIP kernels are shown here, without a GPU, to (a) hold the
classes they claim - every pinned case sits on the branch its label names, every list passes its own coverage assertions on
the restated dispatch, the multiply-add, exactness and frame caps hold -, (b) accept a correct implementation of the contract
in both passes and both precision modes and (c) REJECT implementations that are subtly wrong: each mutant below is a mistake
a conv kernel can make on one path, and the assertion meant for it has to fire."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_cases as CC
from tests import kernel_model as KM

SMALL = 2e7            # multiply-adds of the reduced lists the mutant sweeps run on


def _trunc(t):
    """round toward zero to bf16 precision (the WRONG rounding), kept in fp32"""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _stray(win):
    """one write to the element right behind the last one of the window"""
    last = win.storage_offset() + sum((n - 1) * st for n, st in zip(win.shape, win.stride()))
    win.as_strided((1,), (1,), last + 1).fill_(1.0)


def _scatter_weight(wp, C, O, K, s, pad, aligned, phase_off=0):
    """[C, O, K] from the scatter layout (kernel_model.conv_engine's reading; phase_off: the mutant's wrong phase)"""
    mt, mp = (K + s - 1) // s, KM._r(O * s, 32)
    v = wp.view(KM._r(C, 2), mt, mp)
    return torch.stack([v[:C, min(k // s + (KM._scatter_shift(s, pad, (k % s + phase_off) % s) if aligned else 0), mt - 1),
                          torch.arange(O) * s + k % s] for k in range(K)], 2)


class Model(object):
    """audiogan_amd.kernels as the CPU model computes it in precision `prec`, or a mutant of it.  `case` / `prec` of the call
    at hand are set by the sweep (a kernel knows its own launch geometry; the model takes it from the plan)."""

    def __init__(self, prec, mutate=None):
        self.prec, self.mutate, self.case = prec, mutate, None
        self.wpa_numel, self.wpb_numel, self.prep_conv_weight = KM.wpa_numel, KM.wpb_numel, KM.prep_conv_weight

    def _rnd(self, t):
        if self.prec != 'bf16':
            return t
        return _trunc(t) if self.mutate == 'truncate' else CC.rnd16(t)

    # -- the engine: linear part by the model, epilogue restated so that a mutant can change one step of it ------------
    def conv_engine(self, x, wp, y, K, stride, pad, mode, bias=None, res=None, lens=None, act=CC.ACT_NONE,
                    slope=CC.LEAKY_SLOPE, accumulate=False, wp_pad=0):
        c, mut = self.case, self.mutate
        B, C, Lin = x.shape
        _, O, Lout = y.shape
        x, wp = self._rnd(x), self._rnd(wp)
        pl = CC.conv_plan(self.prec, c)
        if mut == 'last_chunk' and pl['form'] != 'bf16' and pl['chunks'] > 1 and pl['last'] == 2:
            x = x.clone()
            x[:, (pl['chunks'] - 1) * pl['cc']:] = 0

        def linear(xx):
            out = torch.zeros(B, O, Lout)
            if mut == 'scatter_phase' and mode == 1 and pl['aligned']:
                w = _scatter_weight(wp, C, O, K, stride, pad, True, phase_off=1)
                out.copy_(KM._fit(F.conv_transpose1d(xx, w, None, stride, 0)[:, :, pad:], Lout))
            else:
                KM.conv_engine(xx, wp, out, K, stride, pad, mode, wp_pad=wp_pad)
            return out
        lin = linear(x)
        if mut == 'edge_tap':
            xl = torch.zeros_like(x)
            xl[:, :, Lin - 1] = x[:, :, Lin - 1]
            if mode == 1:
                pos = stride * (Lin - 1) + K - 1 - pad
            else:
                pos = max(0, -((K - 1 - (Lin - 1 + pad)) // stride))
                if not 0 <= Lin - 1 + pad - stride * pos < K:
                    pos = -1
            if 0 <= pos < Lout:
                lin[:, :, pos] -= linear(xl)[:, :, pos]
        before = y.clone()
        v = lin
        if bias is not None:
            v = v + bias.view(1, O, 1)
        if res is not None:
            if act == CC.ACT_LEAKY_GATE and mut != 'gate_adds_res':
                v = torch.where(res > 0, v, v * slope)
            else:
                v = v + res
        if act == CC.ACT_LEAKY:
            v = torch.where(v > 0, v, v * slope)
        if lens is not None:
            ln = lens + 1 if mut == 'lens_off' else lens
            v = v * (torch.arange(Lout).view(1, 1, Lout) < ln.view(B, 1, 1)).float()
        out = v + before if accumulate else v
        if accumulate and bias is not None and mut == 'bias_twice':
            out = out + bias.view(1, O, 1)
        if not accumulate and mut == 'reads_prior':
            out = out + 0.0 * before
        if pl['tail'] and mut in ('tail_unwritten', 'tail_twice'):
            n0 = pl['tail']['n_lo']
            u0 = n0 if mode == 0 else (stride * (n0 - pl['n_lo']) if pl['aligned'] else stride * n0 - pad)
            u0 = max(u0, 0)
            if mut == 'tail_unwritten':
                out[:, :, u0:] = before[:, :, u0:]
            elif accumulate:
                out[:, :, u0:] += v[:, :, u0:]
        y.copy_(out)
        if mut == 'stray_write':
            _stray(y)

    # -- the weight gradient --------------------------------------------------------------------------------------------
    def conv_wgrad(self, sh, lg, dw, K, stride, pad):
        c, mut = self.case, self.mutate
        sh, lg = self._rnd(sh), self._rnd(lg)
        pl = CC.wgrad_plan(self.prec, c)
        if mut == 'last_time_chunk' and pl['tile'] and pl['nchunk'] > 1:
            sh = sh.clone()
            sh[:, :, (pl['nchunk'] - 1) * pl['TC']:] = 0
        if mut == 'left_halo_edge' and pad > 0:
            lg, pad = F.pad(lg, (pad, 0), mode='replicate'), 0
        if mut == 'overwrite':
            dw.zero_()
        KM.conv_wgrad(sh.contiguous(), lg.contiguous(), dw, K, stride, pad)
        if mut == 'stray_write':
            _stray(dw)

    # -- the small kernels ------------------------------------------------------------------------------------------------
    def channel_sum(self, dy, db, accumulate=True):
        KM.channel_sum(dy, db, accumulate)

    def leaky_bwd(self, dy, y, dpre, **kw):
        KM.leaky_bwd(dy, y, dpre, **kw)

    def conv_o1_fwd(self, x, w, bias, y, K_, pad, act=CC.ACT_NONE, slope=CC.LEAKY_SLOPE):
        KM.conv_o1_fwd(self._rnd(x), self._rnd(w), bias, y, K_, pad, act, slope)

    def conv_o1_bwd_data(self, dy, w, dx, K_, pad, accumulate=False):
        KM.conv_o1_bwd_data(self._rnd(dy), self._rnd(w), dx, K_, pad, accumulate)

    def conv_o1_wgrad(self, dy, x, dw, K_, pad):
        KM.conv_o1_wgrad(self._rnd(dy), self._rnd(x), dw, K_, pad)


PASSES = dict(exact=CC.EXACT, real=CC.REAL)
_CACHE = {}


def _prepared(kind, ci, c, pas, rounded):
    """(inputs, float64 reference, floor) of a case, computed once per process and shared by every sweep"""
    key = (kind, ci, pas['name'], rounded)
    if key not in _CACHE:
        inputs, reference, floor = dict(engine=(CC.engine_inputs, CC.engine_reference, CC.engine_floor),
                                        wgrad=(CC.wgrad_inputs, CC.wgrad_reference, CC.wgrad_floor))[kind]
        inp = inputs(c, pas, 1000 + ci)
        _CACHE[key] = (inp, reference(c, pas, inp, rounded), floor(c, pas, inp, rounded) if pas is CC.REAL else None)
    return _CACHE[key]


def _sweep(kind, model, passes=('exact', 'real'), limit=None):
    lst, macs, run = dict(engine=(CC.engine_cases(), CC.engine_macs, CC.run_engine),
                          wgrad=(CC.wgrad_cases(), CC.wgrad_macs, CC.run_wgrad))[kind]
    for ci, (label, c) in enumerate(lst):
        if limit is not None and macs(c) > limit:
            continue
        for pn in passes:
            pas = PASSES[pn]
            inp, ref, floor = _prepared(kind, ci, c, pas, model.prec == 'bf16')
            model.case = c
            got = run(model, c, pas, inp, 'cpu')
            CC.check((label, c), pas, ref, got, floor=floor)


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
@pytest.mark.parametrize('kind', ['engine', 'wgrad'])
def test_checker_accepts_the_model(kind, prec):
    _sweep(kind, Model(prec))


def test_checker_accepts_the_kernel_model_itself():
    """the engine's epilogue is restated in Model so that mutants can change one step of it: kernel_model.conv_engine, the
    model the rest of the suite uses, passes the same checks"""
    class Plain(Model):
        def conv_engine(self, *a, **kw):
            KM.conv_engine(*a, **kw)
    _sweep('engine', Plain('f32'), limit=SMALL)


# (what is mutated, precision mode, the pass that has to catch it, the assertion that has to fire)
ENGINE_MUTANTS = [
    ('edge_tap', 'f32', 'exact', 'exact pass'),             # the last tap of a phase dropped at the right signal edge
    ('edge_tap', 'f32', 'real', 'real pass'),
    ('scatter_phase', 'f32', 'exact', 'exact pass'),        # the aligned scatter's shift off by one phase
    ('tail_unwritten', 'f32', 'exact', 'NaN in the output'),
    ('tail_twice', 'f32', 'exact', 'exact pass'),           # the tail columns written twice under accumulate
    ('last_chunk', 'f32', 'exact', 'exact pass'),           # the last 2-channel chunk dropped
    ('last_chunk', 'f32', 'real', 'real pass'),
    ('lens_off', 'f32', 'exact', 'exact pass'),
    ('gate_adds_res', 'f32', 'exact', 'exact pass'),        # the residual added under the gate
    ('reads_prior', 'f32', 'exact', 'NaN in the output'),   # prior output read at accumulate = 0
    ('bias_twice', 'f32', 'exact', 'exact pass'),           # bias added to the accumulated value twice
    ('stray_write', 'f32', 'exact', 'wrote outside'),       # a store one element past the window
    ('truncate', 'bf16', 'real', 'real pass'),              # bf16 truncation instead of round-to-nearest-even
]
WGRAD_MUTANTS = [
    ('last_time_chunk', 'f32', 'exact', 'exact pass'),
    ('last_time_chunk', 'bf16', 'real', 'real pass'),
    ('left_halo_edge', 'f32', 'exact', 'exact pass'),       # the left halo read as the edge sample instead of 0
    ('overwrite', 'f32', 'exact', 'exact pass'),            # dw = instead of dw +=
    ('stray_write', 'f32', 'exact', 'wrote outside'),
    ('truncate', 'bf16', 'real', 'real pass'),
]


@pytest.mark.parametrize('mutate,prec,pn,match', ENGINE_MUTANTS)
def test_checker_rejects_an_engine_mutant(mutate, prec, pn, match):
    with pytest.raises(AssertionError, match=match):
        _sweep('engine', Model(prec, mutate), passes=(pn,), limit=SMALL)


@pytest.mark.parametrize('mutate,prec,pn,match', WGRAD_MUTANTS)
def test_checker_rejects_a_wgrad_mutant(mutate, prec, pn, match):
    with pytest.raises(AssertionError, match=match):
        _sweep('wgrad', Model(prec, mutate), passes=(pn,), limit=SMALL)


def test_a_mutant_changes_nothing_outside_its_path():
    """each engine mutant is a mistake on ONE path: on a case that does not take that path the mutated model still passes
    (so the rejections above come from the cases meant to catch them, not from a broken mutant)"""
    plain = [(l, c) for l, c in CC.PINNED_ENGINE if l in ('64x128', 'K1')]
    for mutate in ('scatter_phase', 'tail_unwritten', 'tail_twice', 'last_chunk', 'lens_off', 'gate_adds_res', 'bias_twice'):
        model = Model('f32', mutate)
        for ci, (label, c) in enumerate(plain):
            inp = CC.engine_inputs(c, CC.EXACT, ci)
            model.case = c
            CC.check(label, CC.EXACT, CC.engine_reference(c, CC.EXACT, inp), CC.run_engine(model, c, CC.EXACT, inp, 'cpu'))


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_checker_accepts_the_model_of_the_small_kernels(prec):
    model = Model(prec)
    for ci, (label, c) in enumerate(CC.small_cases()):
        rounded = prec == 'bf16' and c.op.startswith('o1')
        for pas in (CC.EXACT, CC.REAL):
            inp = CC.small_inputs(c, pas, 1000 + ci)
            ref = CC.small_reference(c, pas, inp, rounded)
            low = CC.small_reference(c, pas, inp, rounded, dtype=torch.float32)
            got = CC.run_small(model, c, pas, inp, 'cpu')
            assert set(got) == set(ref)
            for k in ref:
                CC.check((label, c, k), pas, ref[k], got[k], floor=CC.floor_of(low[k], ref[k]))


def test_small_kernel_checker_rejects_mutants():
    class Bad(Model):
        def channel_sum(self, dy, db, accumulate=True):
            KM.channel_sum(dy, db, True)                          # accumulate = 0 reads db
        def leaky_bwd(self, dy, y, dpre, lens=None, **kw):
            KM.leaky_bwd(dy, y, dpre, lens=lens + 1 if lens is not None else None, **kw)
        def conv_o1_bwd_data(self, dy, w, dx, K_, pad, accumulate=False):
            KM.conv_o1_bwd_data(dy, w, dx, K_, pad, accumulate)
            L = dx.size(2)
            if pad > 0 and L >= 2:                                # the last sample's halo contribution to its left neighbour dropped
                last, t = torch.zeros(dy.shape), torch.zeros(dx.shape)
                last[:, :, L - 1] = dy[:, :, L - 1]
                KM.conv_o1_bwd_data(last, w, t, K_, pad, False)
                dx[:, :, L - 2] -= t[:, :, L - 2]
    model = Bad('f32')
    for op, match in (('sum', 'NaN in the output'), ('leaky', 'exact pass'), ('o1_bwd', 'exact pass')):
        with pytest.raises(AssertionError, match=match):
            for ci, (label, c) in enumerate(CC.small_cases()):
                if c.op != op:
                    continue
                inp = CC.small_inputs(c, CC.EXACT, 1000 + ci)
                ref = CC.small_reference(c, CC.EXACT, inp)
                got = CC.run_small(model, c, CC.EXACT, inp, 'cpu')
                for k in ref:
                    CC.check((label, c, k), CC.EXACT, ref[k], got[k])


# ---------------------------------------------------------------------------------------------------------------------
# the lists: seeded, capped, and on the branches they claim
# ---------------------------------------------------------------------------------------------------------------------
def test_lists_are_seeded_and_within_their_caps():
    e, w, s = CC.engine_cases(), CC.wgrad_cases(), CC.small_cases()
    assert (e, w, s) == (CC.engine_cases(), CC.wgrad_cases(), CC.small_cases()), 'a generator is not deterministic'
    # the 40 seeded shapes of the earlier fuzz: forward, backward-data, backward-weight
    legacy = CC.legacy_shapes()
    assert len(legacy) == 40 and legacy[0][:8] == ('convT', 24, 70, 4, 1, 0, 7, 1) and legacy[39][:8] == ('convT', 40, 33, 6, 2, 4, 100, 2)
    assert sum(l.startswith('legacy') for l, _ in e) == 80 and sum(l.startswith('legacy') for l, _ in w) == 40
    for lst, macs in ((e, CC.engine_macs), (w, CC.wgrad_macs), (s, CC.small_macs)):
        assert max(macs(c) for _, c in lst) <= CC.MAC_MAX
        assert 2 * sum(macs(c) for _, c in lst) <= CC.MAC_SUM_MAX          # (two passes per GPU test function)
    # exactness of the integer pass: 9 x the reduction length (+ bias, residual, prior output: 9 more) below 2^24
    assert all(9 * (c.C * c.K + 1) < 2 ** 24 for _, c in e)
    assert all(c.B >= 3 for _, c in e if c.o['lens'] == 2) and all(c.B >= 3 for _, c in s if c.op == 'leaky' and c.o['lens'] == 2), \
        'a lens table that is to hold 0, 1 and the full length needs three clips'
    assert CC.LEAKY_SLOPE == KM.LEAKY_SLOPE and (CC.ACT_NONE, CC.ACT_LEAKY, CC.ACT_TANH, CC.ACT_LEAKY_GATE) == \
        (KM.ACT_NONE, KM.ACT_LEAKY, KM.ACT_TANH, KM.ACT_LEAKY_GATE)
    assert all(9 * (c.B * c.Lsh + 1) < 2 ** 24 for _, c in w)
    assert all(9 * (max(c.B * c.L, c.C * max(c.K, 1)) + 1) < 2 ** 24 for _, c in s)
    # frames
    for _, c in e:
        for v, C, L in ((c.o['xv'], c.C, c.Lin), (c.o['yv'], c.O, c.Lout), (c.o['rv'], c.O, c.Lout)):
            g = CC.geom(v, C, L)
            assert (c.B + 2 * g['bpad']) * (C + g['ca'] + g['cb']) * g['pitch'] * 4 <= CC.FRAME_MAX
    for _, c in w:
        for v, C, L in ((c.o['shv'], c.A, c.Lsh), (c.o['lgv'], c.C, c.Llg)):
            g = CC.geom(v, C, L)
            assert (c.B + 2 * g['bpad']) * (C + g['ca'] + g['cb']) * g['pitch'] * 4 <= CC.FRAME_MAX
    for _, c in s:
        g = CC.geom('h', c.C, c.L)
        assert (c.B + 2) * (c.C + 3) * g['pitch'] * 4 <= CC.FRAME_MAX


def test_every_case_yields_a_launch():
    for prec in ('f32', 'bf16'):
        for label, c in CC.engine_cases():
            pl = CC.conv_plan(prec, c)
            assert pl['kernel'] and (pl['form'] == 'c1' or pl['taps'] <= CC.MAX_TAPS), (label, c)
            if c.mode == 0:
                assert (c.Lout - 1) * c.s - c.p < c.Lin, (label, c)
        for label, c in CC.wgrad_cases():
            pl = CC.wgrad_plan(prec, c)
            assert pl['kernel'] and not pl['error'], (label, c)
    for label, c in CC.small_cases():
        assert CC.small_plan(c)['kernel'] and (not c.op.startswith('o1') or 1 <= c.K <= CC.O1_MAXK)


def _pinned(lst, label):
    hits = [c for l, c in lst if l == label]
    assert len(hits) == 1, label
    return hits[0]


def test_pinned_engine_cases_sit_on_their_branches():
    def plan(label, prec='f32'):
        return CC.conv_plan(prec, _pinned(CC.PINNED_ENGINE, label))

    def tiles(label, prec='f32'):
        pl = plan(label, prec)
        return pl['tile'], pl['tail']['tile'] if pl['tail'] else None
    assert tiles('128x128') == ((128, 128), None) and tiles('128x128 mode1') == ((128, 128), None)
    assert tiles('128x128+tail') == ((128, 128), (128, 32)) and plan('128x128+tail')['tail']['n_cnt'] == 12
    assert tiles('half+tail') == ((128, 64), (128, 32))
    assert tiles('64x128+tail') == ((64, 128), (64, 64)) and tiles('64x128+tail acc') == ((64, 128), (64, 64))
    assert tiles('64x128') == ((64, 128), None) and tiles('32x256') == ((32, 256), None)
    assert tiles('128x64 n<=64') == ((128, 64), None) and tiles('128x64 taps2') == ((128, 64), None)
    assert tiles('128x64 taps2', 'bf16') == ((128, 64), None)       # (two tap slots stay half-width in fp32 mode only: here by the grid)
    for label, n in (('tail1', 1), ('tail32', 32)):
        assert plan(label)['tail']['n_cnt'] == n
    assert tiles('tail33') == ((128, 128), None) and plan('tail33')['n_cnt'] == 161
    assert tiles('main0') == ((64, 128), None) and plan('main0')['n_cnt'] == 20
    assert tiles('8 column tiles') == ((64, 128), None) and plan('8 column tiles')['n_cnt'] == 8 * 128 + 3
    assert tiles('7 column tiles') == ((64, 128), (64, 64)) and plan('7 column tiles')['tail']['n_cnt'] == 3
    for label, n in (('n63', 63), ('n65', 65), ('n127', 127), ('n129', 129)):
        assert plan(label)['n_cnt'] == n and plan(label)['tile'] == (128, 64)
    for label, key in (('key1708', 1708), ('key904', 904), ('key702', 702), ('128x128', 301), ('key1608', 1608), ('key804', 804),
                       ('128x64 taps2', 200), ('key300 k17s8', 300), ('128x128 mode1', 300), ('key400', 400), ('stride3', 0),
                       ('stride5', 300), ('taps32', 0), ('K1', 0)):
        assert plan(label)['key'] == key, label
    assert plan('taps32')['taps'] == 32
    for label, form, chunks in (('pipe several', 'pipe', 'several'), ('pipe last2', 'pipe', 'last2'), ('pipe last2 odd C', 'pipe', 'last2'),
                                ('generic one', 'generic', 'one'), ('generic several', 'generic', 'several'),
                                ('generic last2', 'generic', 'last2'), ('solo Lin3', 'solo', 'one'), ('solo Lin1', 'solo', 'one'),
                                ('generic Lin3 m0', 'generic', 'one'), ('generic Lin1 m0', 'generic', 'one'),
                                ('solo half <=128', 'solo', 'last2'), ('solo half 128', 'solo', 'several'),
                                ('solo half >128', 'pipe', 'several'), ('solo+dma cc16', 'solo+dma', 'several'),
                                ('solo+dma cc32', 'solo+dma', 'several'), ('solo+dma full', 'solo+dma', 'one'),
                                ('solo several last2', 'solo', 'last2'), ('solo last2 odd C', 'solo', 'last2'),
                                ('128x128 mode1', 'solo', 'one'), ('full solo last2', 'solo', 'last2'),
                                ('full solo last2 k12', 'solo', 'last2'), ('full solo several', 'solo', 'several'),
                                ('full solo+dma several', 'solo+dma', 'several')):
        c = _pinned(CC.PINNED_ENGINE, label)
        cls = CC.plan_class(plan(label), c)
        assert cls[:2] == (form, chunks), (label, cls)
    assert plan('solo+dma cc16')['cc'] == 16 and plan('solo+dma cc32')['cc'] == 32
    for label in ('solo+dma full', '128x128 mode1', 'full solo last2', 'full solo last2 k12', 'full solo several', 'full solo+dma several'):
        assert plan(label)['tile'] == (128, 128), label
    assert plan('full solo last2 k12')['key'] == 300 and _pinned(CC.PINNED_ENGINE, 'full solo last2').C % 2 == 1
    # bf16 mode takes the full tile for a deep reduction whatever the grid; the bf16 kernel refuses Lin % 4 != 0 and the fp32
    # kernel runs it, solo up to C taps = 512
    lo, hi = plan('bf16 full solo 512', 'bf16'), plan('bf16 full 8-wave 520', 'bf16')
    assert lo['kernel'] == hi['kernel'] == 'conv_engine_kernel<2,2,2,2,4,0>'
    assert (lo['form'], lo['chunks'], lo['last']) == ('solo', 10, 2) and hi['form'] == 'generic'
    assert plan('bf16 full solo 512')['tile'] == (128, 64)          # (fp32 mode: half-width by the grid)
    assert not plan('x misaligned')['xvec'] and not plan('x odd pitch')['xvec'] and plan('x aligned pitched')['xvec']
    # the bf16 kernel
    for label, nw, nbuf in (('bf16 C16', 8, 1), ('bf16 C17', 8, 2), ('bf16 C48 nbuf1', 8, 1), ('bf16 nbuf2', 8, 2), ('bf16 NW16', 16, 2),
                            ('bf16 NW16 + tail', 16, 2)):
        pl = plan(label, 'bf16')
        assert (pl['form'], pl['nw'], pl['nbuf']) == ('bf16', nw, nbuf), (label, pl)
    assert tiles('bf16 NW16 + tail', 'bf16') == ((128, 128), (128, 32)) and tiles('bf16 NW16 + tail') == ((128, 64), None)
    for label in ('bf16 C<16', 'bf16 x unaligned', 'bf16 Lin%4'):
        assert plan(label, 'bf16')['kernel'].startswith('conv_engine_kernel<'), label
    # scatter layouts
    for label, al in (('scatter s4 aligned', True), ('scatter s8 aligned', True), ('scatter s2 aligned', True), ('scatter pad%s==0', False),
                      ('scatter extra slot', False), ('scatter wp_pad 0', False), ('m1 out_pad', True)):
        assert plan(label)['aligned'] == al, label
    assert KM._scatter_aligned(8, 4, 2) is False and _pinned(CC.PINNED_ENGINE, 'scatter wp_pad 0').p % 4
    # the single-channel kernels
    for label in ('c1 fwd', 'c1 fwd 1024'):
        assert plan(label)['kernel'] == 'conv_c1_fwd_kernel<2,7,4>'
    assert plan('c1 fwd')['slabs'] == 2 and plan('c1 fwd 1024')['slabs'] == 1 and plan('c1 fwd 1024')['n_cnt'] == 1024
    for label in ('res', 'acc', 'gate', 'y base', 'y pitch'):
        assert plan('c1 fwd declined ' + label)['kernel'] == 'conv_engine_kernel<1,2,1,4,7,2>', label
    base, bs, cs = CC.strides('h', 16, 150)
    assert base % 4 == 0 and cs % 4 == 2, 'declined by the pitch alone'
    base, bs, cs = CC.strides('m', 16, 150)
    assert base % 4 == 1 and cs % 4 == 0 and bs % 4 == 0, 'declined by the base alone'
    for label in ('c1 bwdx', 'c1 bwdx acc', 'c1 bwdx unaligned layout', 'c1 bwdx unaligned acc'):
        assert plan(label)['kernel'] == 'conv_c1_bwdx_kernel<2,7,4>', label
    assert plan('c1 bwdx')['slabs'] == 2 and plan('c1 bwdx acc')['slabs'] == 2
    for label in ('c1 bwdx declined C513', 'c1 bwdx declined lens'):
        assert plan(label)['kernel'].startswith('conv_engine_kernel<1,2,1,4,4,0>'), label


def test_pinned_wgrad_cases_sit_on_their_branches():
    def plan(label, prec='f32'):
        return CC.wgrad_plan(prec, _pinned(CC.PINNED_WGRAD, label))
    for label, cfg in (('32x128 conv', '1,1,1,4'), ('32x128 convT', '1,1,1,4'), ('64x64 A<=64', '1,1,2,2'), ('64x64 CK<=64', '1,1,2,2'),
                       ('64x64 convT', '1,1,2,2'), ('128x128 conv', '2,2,2,2'), ('128x128 convT', '2,2,2,2'), ('c1 k17 mfma', '1,1,2,2')):
        assert plan(label)['kernel'] == 'conv_wgrad_kernel<%s>' % cfg, label
        assert plan(label, 'bf16')['kernel'] == 'conv_wgrad_bf16_kernel<%s>' % cfg, label
    assert plan('bf16 taken', 'bf16')['bf16']
    for label, why in (('bf16 Lsh%64', 'Lsh%64'), ('bf16 sh unaligned', 'sh unaligned'), ('bf16 Llg%4', 'Llg%4'),
                       ('bf16 lg pitch', 'lg pitch or base'), ('bf16 lg base', 'lg pitch or base'), ('bf16 WB_FL', 'WB_FL')):
        pl = plan(label, 'bf16')
        assert not pl['bf16'] and pl['refusal'] == why, (label, pl)
    c = _pinned(CC.PINNED_WGRAD, 'bf16 Llg%4')
    assert c.Lsh % 64 == 0 and c.Llg % 4 == 3
    assert plan('Lsh<TC')['TC'] == 12 and plan('Lsh<TC')['nchunk'] == 1
    assert plan('Lsh%TC')['nchunk'] == 2 and _pinned(CC.PINNED_WGRAD, 'Lsh%TC').Lsh == 100
    assert plan('gz = total')['gz'] == 3 == plan('gz = total')['nchunk']
    assert plan('gz by grid')['gz'] == 26 and plan('gz by grid')['nchunk'] == 16
    assert plan('128x128 conv')['gz'] == 16 > plan('128x128 conv')['nchunk'] == 8
    for label, name in (('c1 wgrad4', 'conv_c1_wgrad4_kernel<2,7,8>'), ('c1 wgrad4 A ragged', 'conv_c1_wgrad4_kernel<2,7,8>'),
                        ('c1 generic k7 unaligned', 'conv_c1_wgrad_kernel<8,8>'), ('c1 generic k5', 'conv_c1_wgrad_kernel<8,8>'),
                        ('c1 generic k8 s4', 'conv_c1_wgrad_kernel<8,8>')):
        assert plan(label)['kernel'] == name, label
    # the workspace test's shape: 16 slabs wanted, fewer under a short workspace, the documented error below one
    c = CC.WS_CASE
    n_out = c.A * c.C * c.K
    full = CC.wgrad_plan('f32', c)
    assert full['kernel'] == 'conv_wgrad_kernel<2,2,2,2>' and full['gz'] == full['ws_want'] // n_out > 3
    assert CC.wgrad_plan('f32', c, 3 * n_out + 5)['gz'] == 3 and CC.wgrad_plan('f32', c, n_out)['gz'] == 1
    assert CC.wgrad_plan('f32', c, n_out - 1)['error']


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_lists_pass_their_coverage_assertions_on_the_restated_dispatch(prec):
    e = [(l, c, CC.conv_plan(prec, c)) for l, c in CC.engine_cases()]
    CC.assert_engine_coverage(prec, [(l, c, pl['kernel'], pl) for l, c, pl in e])
    w = [(l, c, CC.wgrad_plan(prec, c)) for l, c in CC.wgrad_cases()]
    CC.assert_wgrad_coverage(prec, [(l, c, pl['kernel'], pl) for l, c, pl in w])
    CC.assert_small_coverage([(l, c, CC.small_plan(c)) for l, c in CC.small_cases()])


def test_class_lists_are_complete_against_the_branches_of_the_dispatch():
    """every return of ag_conv1d_engine / ag_conv1d_wgrad and every runtime form of launch_cfg / launch_bf16_nw, enumerated by
    hand from the sources, is taken by some case of the lists (the 2 GiB and LDS refusals excepted: see conv_cases)"""
    f32 = [CC.conv_plan('f32', c) for _, c in CC.engine_cases()]
    b16 = [CC.conv_plan('bf16', c) for _, c in CC.engine_cases()]
    mains = set((pl['tile'], pl['tail']['tile'] if pl['tail'] else None) for pl in f32 if pl['form'] != 'c1')
    assert mains == set([((32, 256), None), ((64, 128), None), ((64, 128), (64, 64)), ((128, 64), None), ((128, 128), None),
                         ((128, 64), (128, 32)), ((128, 128), (128, 32))])
    assert set(pl['form'] for pl in f32) == set(['c1', 'generic', 'pipe', 'solo', 'solo+dma'])
    assert set((pl['nw'], pl['nbuf']) for pl in b16 if pl['form'] == 'bf16') == set([(8, 1), (8, 2), (16, 2)])
    assert set(pl['key'] for pl in f32 if pl['form'] != 'c1') == set(CC.TAP_KEYS + (0,))
    names = set(pl['kernel'] for pl in f32) | set(pl['kernel'] for pl in b16)
    assert CC.engine_kernel_names('bf16') <= names
    for prec in ('f32', 'bf16'):
        w = set(CC.wgrad_plan(prec, c)['kernel'] for _, c in CC.wgrad_cases())
        assert w == CC.wgrad_kernel_names(prec) or prec == 'bf16' and CC.wgrad_kernel_names(prec) <= w
    assert set(CC.small_plan(c)['kernel'] for _, c in CC.small_cases()) == set(
        ['channel_sum_kernel', 'leaky_bwd_kernel', 'conv_o1_fwd_vec_kernel<3>', 'conv_o1_fwd_kernel', 'conv_o1_bwdx_vec3_kernel',
         'conv_o1_bwdx_kernel', 'conv_o1_wgrad_vec3_kernel', 'conv_o1_wgrad_kernel'])


def test_coverage_assertion_fails_when_a_class_is_not_reached():
    def seen(lst, prec='f32'):
        return [(l, c, CC.conv_plan(prec, c)['kernel'], CC.conv_plan(prec, c)) for l, c in lst]
    e = CC.PINNED_ENGINE                    # (the pinned list alone holds every class: the seeded cases only add to it)
    CC.assert_engine_coverage('f32', seen(e))
    CC.assert_engine_coverage('bf16', seen(e, 'bf16'))
    for drop in ('128x128+tail', 'tail1', 'key1608', 'solo+dma cc32', 'full solo several', 'full solo+dma several', 'c1 fwd declined y pitch', 'scatter s8 aligned'):
        with pytest.raises(AssertionError):
            CC.assert_engine_coverage('f32', seen([(l, c) for l, c in e if l != drop]))
    with pytest.raises(AssertionError):
        CC.assert_engine_coverage('bf16', seen([(l, c) for l, c in e if not l.startswith('bf16 NW16')], 'bf16'))
    for drop in ('bf16 full solo 512', 'bf16 full 8-wave 520'):
        with pytest.raises(AssertionError):
            CC.assert_engine_coverage('bf16', seen([(l, c) for l, c in e if l != drop], 'bf16'))
    w = CC.PINNED_WGRAD

    def wseen(lst, prec):
        return [(l, c, CC.wgrad_plan(prec, c)['kernel'], CC.wgrad_plan(prec, c)) for l, c in lst]
    for drop, prec in (('bf16 WB_FL', 'bf16'), ('nchunk > gz', 'f32'), ('c1 k17 mfma', 'f32')):
        with pytest.raises(AssertionError):
            CC.assert_wgrad_coverage(prec, wseen([(l, c) for l, c in w if l != drop], prec))
    with pytest.raises(AssertionError):
        CC.assert_small_coverage([(l, c, CC.small_plan(c)) for l, c in CC.PINNED_SMALL if l != 'sum capped'])
