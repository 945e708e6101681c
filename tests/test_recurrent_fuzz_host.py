"""The recurrent launch fuzz (tests/recurrent_cases.py) against the CPU model of the kernels: the generator, references, runner
and checkers that tests/test_recurrent_fuzz.py turns on the HIP kernels are shown here, without a GPU, to (a) accept a correct
implementation of the contract - tests/kernel_model.py for the layer, an fp32 run of the front's reference for the fronts - and
(b) REJECT implementations that are subtly wrong, each by the assertion it is meant to trip.  Each mutant is a mistake a
recurrent kernel can make on one path: a mask off by one step, a carry, a dropped k column, a K slice summed twice in one
tile, a wrong saved tensor, a missing step of a time sum, a store outside its tensor.  It also shows that every case's bound
is finite and below the ceilings, that the seeded tables hold the required classes, and - where the library loads - that the
classes are what the library's own predicates say at 256 CUs."""
import pytest
import torch

from tests import kernel_model as KM
from tests import recurrent_cases as RC


# ---------------------------------------------------------------------------------------------------------------------
# the layer: mutants of the model, each a small wrapper around the model's functions
# ---------------------------------------------------------------------------------------------------------------------
class Walker(RC.Model):
    """the model's step loops (tests/kernel_model.py lstm_seq_fwd / lstm_seq_bwd, cell by cell through its lstm_cell_fwd /
    lstm_cell_bwd) with the two recurrent products and every mutation point as hooks"""
    kind = None

    def prod_fwd(self, h, w):             # [B,H] x [4H,H]^T
        return h @ w.t()

    def prod_bwd(self, dg, w):            # [B,4H] x [4H,H]
        return dg @ w

    def lstm_seq_fwd_fn(self, pre, whh, c_all, hbuf, y, valid, static=None):
        kind = self.kind
        ndir = len(pre)
        T, B, H4 = pre[0].shape
        H = H4 // 4
        for d in range(ndir):
            w = whh[d]
            if kind == 'drop_k_column':
                w = w.clone()
                w[:, H - 3] = 0
            hbuf[d][0].zero_()
            for k in range(T):
                t = k if d == 0 else T - 1 - k
                hp, hn = hbuf[d][k & 1], hbuf[d][(k + 1) & 1]
                if k > 0:
                    pre[d][t].add_(self.prod_fwd(hp, w))
                if static is not None and not (kind == 'static_after_step_0' and k == 0):
                    pre[d][t].add_(static[d])
                v = valid
                if kind == 'reverse_mask_off_by_one' and d == 1 and valid is not None:
                    v = valid - 1                      # t < valid - 1, i.e. t + 1 < valid
                yt = y[t, :, d * H:(d + 1) * H]
                KM.lstm_cell_fwd(pre[d][t], c_all[d][k], c_all[d][k + 1], h_out=hn, y_out=yt, h_prev=hp, valid=v, t=t)
                if v is not None:
                    pad = (t >= v).view(B, 1).expand(B, H)
                    if kind == 'padded_h_zeroed':
                        hn[pad] = 0
                    if kind == 'padded_c_zeroed':
                        c_all[d][k + 1][pad] = 0
                    if kind == 'padded_y_carries_h':
                        yt[pad] = hn[pad] + (hn[pad] == 0).float() * 1e-3   # (a row that never started carries h = 0)

    def lstm_seq_bwd_fn(self, gates, whh, c_all, dy, dgates, dhbuf, dcbuf, valid):
        kind = self.kind
        ndir = len(gates)
        T, B, H4 = gates[0].shape
        H = H4 // 4
        for d in range(ndir):
            for k in reversed(range(T)):
                t = k if d == 0 else T - 1 - k
                dh = None if k == T - 1 else dhbuf[d][k & 1]
                dcn = None if k == T - 1 else dcbuf[d][(k + 1) & 1]
                dpass = dhbuf[d][(k + 1) & 1]
                cp = c_all[d][k + 1] if kind == 'forget_grad_reads_c_new' else c_all[d][k]
                KM.lstm_cell_bwd(gates[d][t], cp, c_all[d][k + 1], dh, dy[t, :, d * H:(d + 1) * H], dcn, dgates[d][t],
                                 dcbuf[d][k & 1], dh_pass=dpass, valid=valid, t=t)
                if k > 0:
                    dpass.add_(self.prod_bwd(dgates[d][t], whh[d]))
                    if kind == 'k_slice_twice_in_one_tile':        # slice 5 of the 8 K slices, clips 0..15 only
                        ks = slice(5 * H4 // 8, 6 * H4 // 8)
                        dpass[:16].add_(dgates[d][t][:16, ks] @ whh[d][ks])
            if kind == 'zero_length_row_writes_dgates' and valid is not None:
                for b in (valid == 0).nonzero().view(-1).tolist()[:1]:
                    dgates[d][T - 1, b, 1] = 1e-6


class Mutant(Walker):
    def __init__(self, kind):
        self.kind = kind

    def lstm_seq_bwd(self, gates, whh, c_all, dy, dgates, dhbuf, dcbuf, valid, dgsum=None, dg16=None):
        RC.Model.lstm_seq_bwd(self, gates, whh, c_all, dy, dgates, dhbuf, dcbuf, valid, dgsum=None, dg16=dg16)
        T = gates[0].size(0)
        if self.kind == 'dgsum_misses_step_0' and dgsum is not None:
            for d in range(len(gates)):             # step 0 is time 0 forward, time T - 1 in reverse
                dgsum[d].copy_((dgates[d][1:] if d == 0 else dgates[d][:T - 1]).sum(0))
            return True
        if self.kind == 'store_past_the_last_row':
            last = dgates[-1]
            last.as_strided((1,), (1,), last.storage_offset() + last.numel()).fill_(1.0)
        return False


# mutant -> the assertion it must trip (the first words of check_layer's message)
LAYER_MUTANTS = [('reverse_mask_off_by_one', 'out of bound|padded y'), ('padded_c_zeroed', 'out of bound: c_all'),
                 ('padded_y_carries_h', 'padded y is not 0'), ('static_after_step_0', 'out of bound'),
                 ('drop_k_column', 'out of bound'), ('k_slice_twice_in_one_tile', 'out of bound: dgates'),
                 ('forget_grad_reads_c_new', 'out of bound: dgates'), ('dgsum_misses_step_0', 'out of bound: dgsum'),
                 ('zero_length_row_writes_dgates', 'padded dgates is not 0'), ('store_past_the_last_row', 'guard frame')]


@pytest.fixture(scope='module')
def layer_table():
    return RC.layer_cases()


def _layer_sweep(cases, mod):
    """check_layer over `cases`; with a mutant: returns the messages of the cases that failed"""
    failed = []
    for case in cases:
        inp, ref, floor = RC.prepared_layer(case)
        got = RC.run_layer(mod, case, inp, 'cpu')
        try:
            RC.check_layer(case, ref, floor, got)
        except AssertionError as e:
            failed.append(str(e.args[0][0]) if e.args and isinstance(e.args[0], tuple) else str(e))
    return failed


def test_checker_accepts_the_model_on_every_layer_case(layer_table):
    for case in layer_table:
        inp, ref, floor = RC.prepared_layer(case)
        got, again = RC.run_layer(RC.Model(), case, inp, 'cpu'), RC.run_layer(RC.Model(), case, inp, 'cpu')
        ratios = RC.check_layer(case, ref, floor, got, again=again)
        assert max(ratios.values()) <= 1.0 + 1e-9           # (the model against its own floor)
        if case['T'] * case['B'] * case['H'] ** 2 <= 2e6:   # the mutants' walker, unmutated, IS the model
            walked = RC.run_layer(Walker(), case, inp, 'cpu')
            assert all(RC.same_bits(walked[k], got[k]) for k in ('y', 'gates', 'c_all', 'dgates', 'dgsum', 'dg16'))


def test_every_layer_bound_is_finite_and_below_the_ceiling(layer_table):
    lo, hi = 1.0, 0.0
    for case in layer_table:
        _, _, floor = RC.prepared_layer(case)
        assert set(floor) == set(RC.LAYER_OUTPUTS)
        for name, f in floor.items():
            b = RC.bound(RC.MARGIN_MAX, f)
            assert f == f and 0 < f < float('inf') and 0 < b <= RC.CEIL, (case, name, f)
            lo, hi = min(lo, f), max(hi, f)
    # the fp32 model against float64: a few 1e-8 on the smallest tensors, below 1e-6 everywhere
    assert 1e-9 < lo and hi < 2e-6, (lo, hi)


@pytest.mark.parametrize('kind,trips', LAYER_MUTANTS)
def test_layer_checker_rejects_a_mutant(layer_table, kind, trips):
    import re
    small = [c for c in layer_table if c['T'] * c['ndir'] * c['B'] * c['H'] ** 2 <= 2e7]
    failed = _layer_sweep(small, Mutant(kind))
    assert failed, 'no case noticed the mutant'
    assert any(re.match(trips, f) for f in failed), (trips, failed[:5])
    # a reordered fp32 sum is NOT a mutant: see test_a_legitimate_summation_order_stays_inside_the_margin


def test_zeroing_a_padded_rows_h_is_an_equivalent_mutant(layer_table):
    """"a padded row's h is zeroed instead of carried" cannot be rejected by any check of the layer's outputs, and this test
    says why by showing it: lengths mask a PREFIX of the time axis, so the forward direction never reads the h of a row again
    once it is padded, and the reverse direction is padded only before a row's first live step, where the carried h is the
    initial 0.  h is scratch, not an output: every output is bit-identical.  (The cell IS an output, c_all is indexed by step
    and holds the carried value: 'padded_c_zeroed' above is the observable sibling.)"""
    small = [c for c in layer_table if c['T'] * c['ndir'] * c['B'] * c['H'] ** 2 <= 2e7 and c['kind'] in ('ragged', 'tail0')]
    assert len(small) >= 10
    for case in small:
        inp, ref, _ = RC.prepared_layer(case)
        a, b = RC.run_layer(Mutant('padded_h_zeroed'), case, inp, 'cpu'), RC.run_layer(RC.Model(), case, inp, 'cpu')
        assert all(RC.same_bits(a[k], b[k]) for k in ('y', 'c_all', 'dgates', 'dgsum', 'dg16'))
        live = ref['live'].view(case['T'], case['B'], 1)          # (gates at padded steps: unspecified by the contract)
        assert all(RC.same_bits(torch.where(live, x, torch.zeros(())), torch.where(live, y_, torch.zeros(())))
                   for x, y_ in zip(a['gates'], b['gates']))


def _in_8_slices(x, w):
    K_ = x.size(1)
    e = [K_ * i // 8 for i in range(9)]
    out = x[:, e[0]:e[1]] @ w[e[0]:e[1]]
    for i in range(1, 8):
        out = out + x[:, e[i]:e[i + 1]] @ w[e[i]:e[i + 1]]
    return out


class EightSlices(Walker):
    """the model with both recurrent products summed as the kernels sum them: 8 K slices, each in fp32, added in turn"""

    def prod_fwd(self, h, w):
        return _in_8_slices(h, w.t())

    def prod_bwd(self, dg, w):
        return _in_8_slices(dg, w)


def test_a_legitimate_summation_order_stays_inside_the_margin(layer_table):
    """the reason for a margin at all: the same fp32 arithmetic in another order of summation passes"""
    small = [c for c in layer_table if c['T'] * c['ndir'] * c['B'] * c['H'] ** 2 <= 2e7]
    worst = 0.0
    for case in small:
        inp, ref, floor = RC.prepared_layer(case)
        ratios = RC.check_layer(case, ref, floor, RC.run_layer(EightSlices(), case, inp, 'cpu'))
        worst = max(worst, max(ratios.values()))
    assert worst < RC.MARGIN


def test_layer_reference_states_the_masked_step_contract():
    """the float64 reference on a hand-checked case: a zero-length row gives y = 0, c = 0 at every step and dgates = 0; a row
    of length 1 has its only live step at time 0 in BOTH directions, the reverse one starting there from h = c = 0; c_all is
    indexed by step"""
    T, B, H = 3, 3, 8
    gen = torch.Generator().manual_seed(3)
    pre = [torch.randn(T, B, 4 * H, generator=gen) for _ in range(2)]
    whh = [torch.randn(4 * H, H, generator=gen) / H ** 0.5 for _ in range(2)]
    dy = torch.randn(T, B, 2 * H, generator=gen)
    valid = torch.tensor([3, 1, 0])
    r = RC.ref_lstm_layer(pre, whh, valid, None, dy)
    assert not bool(r['y'][:, 2].any()) and not bool(r['c_all'][0][:, 2].any()) and not bool(r['dgates'][1][:, 2].any())
    assert not bool(r['y'][1:, 1].any())
    for d in range(2):          # row 1: one live step from zero state, the same algebra in both directions
        g = pre[d][0, 1].double()
        i, gg, o = torch.sigmoid(g[:H]), torch.tanh(g[2 * H:3 * H]), torch.sigmoid(g[3 * H:])
        assert torch.allclose(r['y'][0, 1, d * H:(d + 1) * H], o * torch.tanh(i * gg), atol=1e-14, rtol=0)
    # forward: row 1's cell is set at step 0 and carried; reverse: it stays 0 until step 2 (time 0)
    assert bool(r['c_all'][0][1, 1].any()) and torch.equal(r['c_all'][0][1, 1], r['c_all'][0][3, 1])
    assert not bool(r['c_all'][1][:3, 1].any()) and bool(r['c_all'][1][3, 1].any())
    assert torch.allclose(r['dgsum'][0], r['dgates'][0].sum(0))


# ---------------------------------------------------------------------------------------------------------------------
# AG_PREC_BF16: the teacher-forced step checks on a CPU statement of the mode
# ---------------------------------------------------------------------------------------------------------------------
class RoundedModel(Walker):
    """the model with both operands of the recurrent products rounded to bf16 (RNE), or truncated / not rounded (mutants)"""

    def __init__(self, fwd='rne', bwd='rne'):
        how = dict(rne=RC.rnd, none=lambda t: t, trunc=lambda t: (t.contiguous().view(torch.int32) & -65536).view(torch.float32))
        self.rf, self.rb = how[fwd], how[bwd]

    def prod_fwd(self, h, w):
        return self.rf(h) @ self.rf(w).t()

    def prod_bwd(self, dg, w):
        return self.rb(dg) @ self.rb(w)


def _tf_sweep(cases, mod):
    for case in cases:
        inp, ref, _ = RC.prepared_layer(case)
        got = RC.run_layer(mod, case, inp, 'cpu', options=False)
        RC.check_tf(case, inp, got, ref['live'], ('model', 'model'))


def test_teacher_forced_checks_accept_rounding_and_reject_its_absence(layer_table):
    small = [c for c in layer_table if c['T'] * c['ndir'] * c['B'] * c['H'] ** 2 <= 2e7]
    assert any(c['T'] == 2 and c['H'] >= 64 for c in small) and any(c['T'] > 2 for c in small)
    _tf_sweep(small, RoundedModel('rne'))
    # (an implementation that does not round, or truncates, is first of all far from the rounded reference: the bound trips;
    # "did not round" guards the other way round, a reference that stopped rounding)
    with pytest.raises(AssertionError, match='out of bound: gates'):
        _tf_sweep(small, RoundedModel('none'))
    with pytest.raises(AssertionError, match='out of bound: gates'):
        _tf_sweep(small, RoundedModel('trunc'))
    # the backward product alone (T = 2 cases reach it)
    for how in ('none', 'trunc'):
        with pytest.raises(AssertionError, match='out of bound: dgates'):
            _tf_sweep([c for c in small if c['T'] == 2], RoundedModel('rne', how))


# ---------------------------------------------------------------------------------------------------------------------
# fronts
# ---------------------------------------------------------------------------------------------------------------------
def _front_model(cell, inp, mutate=None):
    got = RC.ref_front(cell, inp['zc'], inp['vg'], inp['gx'], inp['gs'], dtype=torch.float32, mutate=mutate)
    got['frames_ok'] = True
    return got


@pytest.mark.parametrize('cell', ['lstm', 'gru'])
def test_front_checker_accepts_the_fp32_reference_and_bounds_stay_below_the_ceilings(cell):
    for case in RC.front_cases():
        inp, ref, floor = RC.prepared_front(case, cell)
        RC.check_front(case, inp, ref, floor, _front_model(cell, inp), again=_front_model(cell, inp))
        for name, f in floor.items():
            ceil = RC.CEIL_GRAD_L2 if name.endswith('.l2') else RC.CEIL_GRAD_ELEM if name.endswith('.elem') else RC.CEIL
            assert f == f and f < float('inf') and RC.bound(RC.MARGIN_MAX, f, ceil) <= ceil, (case, name, f)


@pytest.mark.parametrize('cell,mutate,trips', [('lstm', 'xprev_is_x0', 'out of bound: x'), ('gru', 'xprev_is_x0', 'out of bound: x'),
                                               ('gru', 'bhn_outside', 'out of bound: x'), ('lstm', 'stop_prev', 'out of bound: s'),
                                               ('gru', 'stop_prev', 'out of bound: s')])
def test_front_checker_rejects_a_mutant(cell, mutate, trips):
    hit = 0
    for case in [c for c in RC.front_cases() if c['S'] == 128]:
        inp, ref, floor = RC.prepared_front(case, cell)
        with pytest.raises(AssertionError, match=trips):
            RC.check_front(case, inp, ref, floor, _front_model(cell, inp, mutate))
        hit += 1
    assert hit >= 10        # EVERY case notices: T = 1 included (x_{-1}, the stop logit of frame 0)


def test_front_checker_notices_a_stray_store_and_a_changed_second_call():
    case = RC.front_cases()[1]
    inp, ref, floor = RC.prepared_front(case, 'lstm')
    got = _front_model('lstm', inp)
    with pytest.raises(AssertionError, match='guard frame'):
        RC.check_front(case, inp, ref, floor, dict(got, frames_ok=False))
    other = dict(got, x=got['x'].clone())
    other['x'][0, 0] += 1e-7
    with pytest.raises(AssertionError, match='not reproducible'):
        RC.check_front(case, inp, ref, floor, got, again=other)
    f = RC.Framed((3, 5), 'cpu')
    assert f.intact()
    f.flat[RC.GUARD + 15] = 1.0          # the element right behind the window
    assert not f.intact()


# ---------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------
def test_case_tables_are_seeded_and_hold_the_required_classes(layer_table):
    assert layer_table == RC.layer_cases() and RC.front_cases() == RC.front_cases(), 'the generator is not deterministic'
    assert RC.layer_cases(seed=62) != layer_table
    RC.assert_layer_classes(layer_table)
    RC.assert_front_classes(RC.front_cases())
    with pytest.raises(AssertionError):
        RC.assert_layer_classes([c for c in layer_table if c['H'] != 704])
    with pytest.raises(AssertionError):
        RC.assert_layer_classes([c for c in layer_table if c['kind'] != 'tail0' or c['cls'] != 'bwd'])
    with pytest.raises(AssertionError):
        RC.assert_layer_classes([c for c in layer_table if c['T'] != RC.T_LONG])
    with pytest.raises(AssertionError):
        RC.assert_front_classes([c for c in RC.front_cases() if c['fs'] != 200])
    for c in layer_table:
        v = RC.make_layer_inputs(c)['valid']
        if c['kind'] == 'none':
            assert v is None
        elif c['kind'] == 'full':
            assert bool((v == c['T']).all())
        else:
            assert int(v[0]) == c['T'] and int(v.min()) >= 0 and int(v.max()) <= c['T']
            if c['B'] >= 4:
                assert v[1:4].tolist() == [0, 1, c['T']]
        if c['kind'] == 'tail0':
            tile = 16 if c['cls'] == 'bwd' and c['B'] <= 32 else 32
            z0 = tile * ((c['B'] - 1) // tile)
            assert z0 > 0 and not bool(v[z0:].any()), c


def test_classes_are_what_the_library_says_at_256_cus(layer_table):
    """(host coverage: libaudiogan_hip.so loads without a GPU, as tests/test_host_logic.py uses it)"""
    from audiogan_amd._lib import lib
    for c in layer_table:
        B, H, ndir = c['B'], c['H'], c['ndir']
        fwd, bwd = RC.layer_forms(c)
        assert bool(lib.ag_lstm_persist_ok(B, H, ndir, 256)) == fwd.startswith('fwd_persist'), c
        assert bool(lib.ag_lstm_persist_bwd_ok(B, H, ndir, 256)) == bwd.startswith('bwd_persist'), c
        if fwd == 'fwd_persist<1>':       # 32-clip tiles: the 32-clip grid itself fits
            assert ndir * ((B + 31) // 32) * (H // 8) <= 256
    for c in RC.front_cases():
        assert lib.ag_gfront_persist_ok(c['B'], c['S'], c['fs'], 256) and lib.ag_gfront_bwd_persist_ok(c['B'], c['S'], c['fs'], 256), c
