"""The pointwise and reduction launch fuzz (tests/pointwise_cases.py) against the CPU model of the kernels: the case lists,
plans, runners, float64 references and checker that tests/test_pointwise_fuzz.py turns on the HIP kernels are shown here,
without a GPU, to (a) pass their own coverage assertions, (b) accept a correct implementation of every contract in every
pass and (c) REJECT implementations that are subtly wrong: each mutant below is a mistake one of these kernels can make on
one path, and the assertion meant for it has to fire."""
import re

import pytest
import torch

from tests import kernel_model as KM
from tests import pointwise_cases as PC


Model = PC.CpuModel


@pytest.mark.parametrize('fam', sorted(PC.FAMILIES))
def test_checker_accepts_the_model(fam):
    PC.sweep(fam, Model(), 'cpu')


def test_checker_accepts_the_model_in_bf16_mode():
    PC.sweep('rd', Model('bf16'), 'cpu', prec='bf16')


def test_the_unrounded_model_fails_in_bf16_mode():
    """the bf16-mode reference rounds what the kernel rounds: an implementation that does not round is out of bound"""
    with pytest.raises(AssertionError, match='real pass: out of bound'):
        PC.sweep('rd', Model('f32'), 'cpu', prec='bf16', passes=('real',), only=lambda l, c: c.op == 'rowdot' and not c.x16)


def test_closed_form_time_moment_gradient_is_the_derivative_of_the_forward():
    """tm_reference states the backward in the closed form the kernel documents; here it is held, in float64, against
    autograd of the forward definition (kernel_model.time_moments_bwd) on every case - all-zero rows included, where both
    keep the gm term alone"""
    for ci, (label, c) in enumerate(PC.tm_cases()):
        inp = PC.tm_inputs(c, PC.REAL, 1000 + ci)
        ref = PC.tm_reference(c, PC.REAL, inp, torch.float64)['dh']
        g = [(inp[k].double() if k not in c.absent else None) for k in ('gm', 'gs', 'gf')]
        dh = torch.empty(c.B, c.C, c.L, dtype=torch.float64)
        KM.time_moments_bwd(inp['h'].double(), inp['lens'], g[0], g[1], g[2], dh)
        tol = 1e-6 if c.tight_row else 1e-11           # (float64 on a row of mean 100 and spread 0.01: 1e4^2 x 2^-53 per term)
        assert float((dh - ref).abs().max()) <= tol * float(ref.abs().max()), (label, float((dh - ref).abs().max()))


def _trunc(t):
    """round toward zero to bf16 precision (the WRONG rounding), kept in fp32"""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _stray(win):
    """one write to the element right behind the last one of the window"""
    last = win.storage_offset() + sum((n - 1) * st for n, st in zip(win.shape, win.stride()))
    win.as_strided((1,), (1,), last + 1).fill_(1.0)


class Mutant(Model):
    """one mistake per name; every other call is the model's"""

    # -- weight norm ---------------------------------------------------------------------------------------------------
    def weight_norm_fwd(self, entries):
        mut = self.mutate
        if mut == 'wn_shift_unaligned':
            keep = [e['wpb'].clone() if e.get('wpb') is not None else None for e in entries]
        Model.weight_norm_fwd(self, entries)
        for i, e in enumerate(entries):
            rows, cols, d1, K = PC._wn_dims(tuple(e['v'].shape))
            w = e.get('w')
            if mut == 'wn_norm_short' and cols > 1 and w is not None:         # the norm over cols - 1 elements
                v2 = e['v'].reshape(rows, -1)
                w.copy_((w.reshape(rows, -1) * (v2.norm(dim=1, keepdim=True) / v2[:, :-1].norm(dim=1, keepdim=True))).view(w.shape))
            if mut == 'wn_tail_dropped' and cols > 64 and w is not None:      # a lane loop that stops after one round
                w.view(rows, -1)[:, 64:] = float('nan')
            if mut == 'wn_shift_unaligned' and keep[i] is not None:
                s, pad = int(e.get('stride', 1)), int(e.get('pad', 0))
                if s > 1 and pad % s and not PC.scatter_aligned(K, s, pad):
                    ed = dict(rows=rows, d1=d1, K=K, s=s, pad=pad, aligned=False)
                    good = PC.wn_maps(ed)['b'][1]
                    bad = PC.wn_maps(dict(ed, aligned=True))['b'][1].clamp(max=keep[i].numel() - 1)
                    vals = e['wpb'][good]
                    e['wpb'].copy_(keep[i])
                    e['wpb'][bad] = vals

    # -- cells -----------------------------------------------------------------------------------------------------------
    def lstm_cell_fwd(self, gates, c_prev, c_out, h_out=None, y_out=None, h_prev=None, valid=None, t=0):
        g0 = gates.clone()
        KM.lstm_cell_fwd(gates, c_prev, c_out, h_out, y_out, h_prev, valid, t)
        if valid is None:
            return
        pad = t >= valid
        if self.mutate == 'lstm_pad_gates':
            H = g0.size(1) // 4
            act = torch.cat([torch.sigmoid(g0[:, :2 * H]), torch.tanh(g0[:, 2 * H:3 * H]), torch.sigmoid(g0[:, 3 * H:])], 1)
            gates[pad] = act[pad]
        if self.mutate == 'lstm_h_zeroed' and h_out is not None:
            h_out[pad] = 0.0

    def lstm_cell_bwd(self, gates_act, c_prev, c_new, *a, **kw):
        KM.lstm_cell_bwd(gates_act, c_new if self.mutate == 'lstm_f_cnew' else c_prev, c_new, *a, **kw)

    def gru_cell_bwd(self, gates_act, gh, h_prev, dh, dgi, dgh, dh_prev):
        KM.gru_cell_bwd(gates_act, gh, h_prev, dh, dgi, dgh, dh_prev)
        if self.mutate == 'gru_dghn_no_r':
            H = dgi.size(1) // 3
            dgh[:, 2 * H:] = dgi[:, 2 * H:]

    # -- losses ----------------------------------------------------------------------------------------------------------
    def bce_logits_fwd(self, x, target, nframes, per_sample, loss, scale):
        if self.mutate != 'bce_div_T':
            return KM.bce_logits_fwd(x, target, nframes, per_sample, loss, scale)
        KM.bce_logits_fwd(x, target, nframes, per_sample, None, scale)
        loss.add_(scale * (per_sample / x.size(1)).sum())

    def bce_logits_fwd_strided(self, x, target, nframes, per_sample, loss, scale, target_rows=None):
        l0 = loss.clone()
        KM.bce_logits_fwd_strided(x, target, nframes, per_sample, loss, scale, None if self.mutate == 'bce_rows_ignored' else target_rows)
        if self.mutate == 'bce_strided_acc':
            loss.add_(l0)

    def bce_logits_bwd_strided(self, x, target, nframes, gscale, scale, dx, target_rows=None):
        KM.bce_logits_bwd_strided(x, target, nframes, gscale, scale, dx, None if self.mutate == 'bce_rows_ignored' else target_rows)

    # -- elementwise -------------------------------------------------------------------------------------------------------
    def act_bwd(self, dy, y, dx, act, slope=PC.LEAKY_SLOPE):
        if self.mutate == 'leaky_zero_pos' and act == PC.ACT_LEAKY:
            return dx.copy_(torch.where(y >= 0, dy, dy * slope))
        KM.act_bwd(dy, y, dx, act, slope)

    def axpby(self, x, y, a, b):
        if self.mutate == 'axpby_nan':
            return y.copy_(a * x + b * y)
        KM.axpby(x, y, a, b)

    def critic_batch(self, xa, na=None, xb=None, nb=None, len_a=None, len_b=None, prods=(), ca=None, cb=None):
        x, tab, c = KM.critic_batch(xa, na, xb, nb, len_a, len_b, prods, ca, cb)
        if self.mutate == 'critic_floor' and tab is not None:
            L = xa.size(1)
            ln = torch.cat([l if l is not None else torch.full((n,), L, dtype=torch.int64)
                            for l, n in ((len_a, xa.size(0)), (len_b, xb.size(0) if xb is not None else 0))])
            tab = torch.stack([ln // d for d in prods], 0)
        return x, tab, c

    # -- optimiser -----------------------------------------------------------------------------------------------------------
    def grad_norms(self, params, grads, s1, s2, norms, norm_sum, flags, grad_scale=1.0, step_dev=None, finish=True):
        old = flags.clone()
        r = Model.grad_norms(self, params, grads, s1, s2, norms, norm_sum, flags, grad_scale, step_dev, finish)
        if self.mutate == 'big_before_scale':
            f = int(flags) & 1
            flags.fill_(f | (2 if any(bool((g.abs() > 1e5).any()) for g in grads) else 0))
        if self.mutate == 'flags_ored':
            flags.copy_(flags | old)
        return r

    def opt_step(self, params, grads, s1, s2, norms, kind, lr, clip, grad_scale, a1, b2, eps, step, step_dev=None, part=None,
                 norm_sum=None, flags=None):
        if self.mutate == 'clip_always' and clip > 0:          # the clip applied at norm < clip as well
            grads = [g / (float(n) / PC.f32(clip)) if float(n) <= clip else g for g, n in zip(grads, norms)]
        if self.mutate == 'adam_step_minus1' and kind == PC.OPT_ADAM:
            if step_dev is not None:
                step_dev = step_dev - 1
            elif step == 1:                                    # 1 - beta^0 = 0: the C arithmetic divides by it
                for p in params:
                    p.fill_(float('inf'))
                return
            else:
                step -= 1
        Model.opt_step(self, params, grads, s1, s2, norms, kind, lr, clip, grad_scale, a1, b2, eps, step, step_dev, part, norm_sum, flags)

    # -- time moments -----------------------------------------------------------------------------------------------------------
    def time_moments_fwd(self, h, lens, m, s, f):
        if self.mutate != 'tm_center_padded':
            return KM.time_moments_fwd(h, lens, m, s, f)
        lf = lens.view(-1, 1).float()
        mm = h.sum(2) / lf
        cen = h - mm.unsqueeze(2)                              # the mean subtracted at the padded steps too
        m.copy_(mm); s.copy_((cen ** 2).sum(2) ** 0.5 / lf); f.copy_((cen ** 4).sum(2) ** 0.25 / lf)

    def time_moments_bwd(self, h, lens, gm, gs, gf, dh):
        KM.time_moments_bwd(h, lens, gm, gs, gf, dh)
        if self.mutate == 'tm_zero_row_nan' and gs is not None:
            dh[(h.abs().sum(2) == 0)] = float('nan')           # sqrt'(0): the term kept

    # -- transposes ---------------------------------------------------------------------------------------------------------------
    def _narrow(self, r, out):
        if self.mutate == 'tr_truncate' and out.dtype == torch.bfloat16 and r.dtype == torch.float32:
            r = _trunc(r)
        out.copy_(r.reshape(out.shape))
        if self.mutate == 'tr_edge_past':
            _stray(out)
        return out

    def bct_to_tbc(self, x, out=None, out_dtype=None):
        return self._narrow(x.permute(2, 0, 1).contiguous(), out)

    def tbc_to_bct(self, x, out=None, out_dtype=None):
        return self._narrow(x.permute(1, 2, 0).contiguous(), out)

    def to_bf16(self, src, out=None):
        return self._narrow(src.contiguous(), out)

    # -- one-output Linear, column sums ---------------------------------------------------------------------------------------------
    def rowdot_bwd(self, dy, x, w, dx=None, dw=None, db=None, **kw):
        db0 = db.clone() if db is not None else None
        Model.rowdot_bwd(self, dy, x, w, dx, dw, db, **kw)
        if self.mutate == 'rowdot_db_skipped' and db is not None and x.size(1) > 256:
            db.copy_(db0)                                      # `k == 0` taken per tile: no thread of the second tile has it ...

    def col_sum(self, X, out, accumulate=True, defer=True):
        KM.col_sum(X, out, accumulate, defer)
        if self.mutate == 'colsum_block_twice' and X.size(0) > 16:
            out.add_(X[:16].float().sum(0))

    # -- Conv2DLSTM, layer norm -----------------------------------------------------------------------------------------------------
    def convlstm_peephole_fwd(self, y, c, wci, wcf, j, ip, fp, o):
        KM.convlstm_peephole_fwd(y, c, wci, wcf, j, ip, fp, o)
        if self.mutate == 'peep_w_by_batch' and wci is not None:
            H, B, F, W = c.shape
            ip.copy_(y[:, :, F:2 * F] + wci[torch.arange(B) % H].unsqueeze(0) * c)

    def layer_norm_hbfw_fwd(self, x, gamma, beta, eps, y, mean, rstd):
        KM.layer_norm_hbfw_fwd(x, gamma, beta, eps, y, mean, rstd)
        if self.mutate == 'ln_var_uncentred':
            rstd.copy_(torch.rsqrt((x ** 2).mean(dim=(0, 2, 3)) - mean ** 2 + eps).nan_to_num(1e6))     # E[x^2] - m^2

    def layer_norm_hbfw_bwd(self, dy, x, gamma, mean, rstd, dx, dgp, dbp):
        KM.layer_norm_hbfw_bwd(dy, x, gamma, mean, rstd, dx, dgp, dbp)
        if self.mutate == 'ln_dgamma_no_rstd':
            dgp.copy_((dy * (x - mean.view(1, -1, 1, 1))).sum(dim=(0, 3)).view(dgp.shape))


OOB, NANOUT, BITS, EXACT_, INT_, OUTSIDE = ('real pass: out of bound', 'NaN in the output', 'output differs in its bits from the reference',
                                            'exact pass: output differs from the float64 reference', 'integer output differs from the reference',
                                            'wrote outside its window')
# (what is mutated, family, the assertion that has to fire, the output it has to fire on)
MUTANTS = [
    ('wn_norm_short', 'wn', OOB, r'w\.\d+'),                   # weight-norm norm over cols - 1 elements
    ('wn_tail_dropped', 'wn', NANOUT, r'w\.\d+'),              # a row tail beyond 64 columns dropped
    ('wn_shift_unaligned', 'wn', OUTSIDE, r'wpb\.8'),          # wpb shift applied when the layout is not aligned (entry 8: k = 2 s)
    ('lstm_pad_gates', 'cells', BITS, 'gates_pad'),           # a padded LSTM row whose gates are overwritten
    ('lstm_h_zeroed', 'cells', BITS, 'h_out_pad'),            # h zeroed, not carried, at a padded step
    ('lstm_f_cnew', 'cells', OOB, 'dgates'),                  # the forget-gate gradient reading c_new
    ('gru_dghn_no_r', 'cells', OOB, 'dgh'),                   # GRU dgh_n without r
    ('bce_div_T', 'bce', OOB, 'loss'),                        # BCE divided by T where it should be n
    ('bce_strided_acc', 'bce', NANOUT, 'loss'),               # the strided loss accumulated where it should be written
    ('bce_rows_ignored', 'bce', OOB, 'loss'),                 # target rows ignored
    ('leaky_zero_pos', 'elem', EXACT_, 'dx'),                 # the leaky gate taking 0 as positive
    ('axpby_nan', 'elem', NANOUT, 'y'),                       # axpby propagating NaN at b == 0
    ('critic_floor', 'elem', INT_, 'lens'),                   # floor in place of ceil in critic_batch lengths
    ('clip_always', 'opt', OOB, 'p'),                         # the clip applied at norm < clip
    ('big_before_scale', 'opt', INT_, 'flags'),               # the BIG flag tested before grad_scale
    ('flags_ored', 'opt', INT_, 'flags'),                     # flags OR-ed into the old word
    ('adam_step_minus1', 'opt', OOB, 'p'),                    # Adam's correction with step - 1
    ('tm_center_padded', 'tm', OOB, 's'),                     # moments centred over padded steps
    ('tm_zero_row_nan', 'tm', NANOUT, 'dh'),                  # the zero-row term kept (NaN)
    ('tr_edge_past', 'tr', OUTSIDE, 'y'),                     # a transposed tile edge stored past R (frame)
    ('tr_truncate', 'tr', 'bf16 output is not RNE', 'y'),     # truncation in place of round-to-nearest-even
    ('rowdot_db_skipped', 'rd', NANOUT, 'dwb'),               # rowdot db skipped when k == 0 lies in a second tile
    ('colsum_block_twice', 'rd', EXACT_, 'out'),              # a col_sum row block summed twice
    ('ln_var_uncentred', 'cl', OOB, 'rstd'),                  # layer-norm variance uncentred
    ('ln_dgamma_no_rstd', 'cl', OOB, 'dgp'),                  # dgamma without rstd
    ('peep_w_by_batch', 'cl', EXACT_, 'ip'),                  # peephole weights indexed by batch where the row index belongs
]


@pytest.mark.parametrize('mutate,fam,what,output', MUTANTS)
def test_checker_rejects_a_mutant(mutate, fam, what, output):
    """the first assertion to fire is the one meant for the mutant, on the output it corrupts"""
    with pytest.raises(AssertionError, match="%s.*\\('%s', '[^']*', '%s'\\)" % (re.escape(what), fam, output)):
        PC.sweep(fam, Mutant(mutate=mutate), 'cpu')


def test_a_mutant_changes_nothing_outside_its_family():
    """each mutant is a mistake in ONE kernel: the mutated model still passes the other families (so the rejections above
    come from the cases meant to catch them, not from a broken mutant)"""
    for mutate, fam, _, _ in MUTANTS:
        for other in ('wn', 'cells', 'bce', 'tm', 'tr'):
            if other != fam:
                PC.sweep(other, Mutant(mutate=mutate), 'cpu')


def test_vacuous_references_fail():
    """a real pass whose float64 reference is all zero fails as vacuous, and no case of the lists has such a reference (the
    sweeps above pass on the reference's own inputs)"""
    ref = torch.zeros(4, dtype=torch.float64)
    got = dict(out=torch.zeros(4), frame_ok=True, kernel='k')
    with pytest.raises(AssertionError, match='all zero'):
        PC.pcheck('t', PC.REAL, ref, got, low=torch.zeros(4))
    got16 = dict(out=torch.zeros(4, dtype=torch.bfloat16), frame_ok=True, kernel='k')
    with pytest.raises(AssertionError, match='all zero'):
        PC.pcheck('t', PC.REAL, ref, got16, low=torch.zeros(4))


def test_lists_are_deterministic_and_exact_passes_stay_exact():
    for fam in PC.ORDER:
        F = PC.FAMILIES[fam]
        assert F.cases() == F.cases(), fam
        assert len(set(l for l, _ in F.cases())) == len(F.cases()), ('labels are unique', fam)
    # reduction length x largest product below 2^24 wherever a sum is compared bit for bit
    assert all(9 * max(c.K, c.M) < 2 ** 24 for _, c in PC.rd_cases() if c.op == 'rowdot')
    assert all(3 * c.M < 2 ** 24 for _, c in PC.rd_cases() if c.op == 'col_sum')
    assert all(9 * c.shape[1] < 2 ** 24 and 3 * c.shape[0] * c.shape[3] < 2 ** 24 for _, c in PC.cl_cases())
    assert all(n * m * m < 2 ** 24 and round((n * m * m) ** 0.5) ** 2 == n * m * m for n, m in PC.EXACT_MAG.items())
    assert PC.LEAKY_SLOPE == KM.LEAKY_SLOPE and (PC.OPT_RMSPROP, PC.OPT_ADAM) == (KM.OPT_RMSPROP, KM.OPT_ADAM)


def test_coverage_assertion_fails_when_a_class_is_not_reached():
    for fam, drop in (('elem', lambda l: 'L2305' in l), ('cells', lambda l: 'H600' in l), ('bce', lambda l: 'B33' in l),
                      ('opt', lambda l: 'flag inf' in l), ('tm', lambda l: 'zero-row' in l), ('tr', lambda l: 'pitched' in l),
                      ('rd', lambda l: 'wbase' in l), ('cl', lambda l: 'mean1000' in l), ('wn', lambda l: l.startswith('one '))):
        F = PC.FAMILIES[fam]
        seen = [(l, c, F.plan(c, 'f32')) for l, c in F.cases()]
        F.coverage(seen)
        with pytest.raises(AssertionError, match='never reached'):
            F.coverage([s for s in seen if not drop(s[0])])
