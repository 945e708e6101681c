"""The statistics launch fuzz (tests/stats_cases.py) against the CPU models of the kernels: the case lists, plans, runners,
float64 references and checks that tests/test_stats_fuzz.py turns on the HIP kernels are shown here, without a GPU, to (a)
pass their own coverage assertions, (b) accept the models in every pass, (c) agree with values worked out by hand on
three-element cases and (d) REJECT implementations that are subtly wrong: each mutant below is a mistake one of these kernels
can make on one branch, and the assertion meant for it has to fire.  The launchers' refusals are host code and are checked
here too."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

from tests import eval_model as EM
from tests import stats_cases as SC
from tests import summary_model as SM

EXACT, REAL, Case = SC.EXACT, SC.REAL, SC.Case


@pytest.mark.parametrize('fam', SC.ORDER)
def test_checker_accepts_the_models(fam):
    worst = {}
    SC.sweep(fam, SC.CpuModel(), 'cpu', worst=worst)
    for k in sorted(worst):
        print('  %-64s %6.2f' % (k, worst[k]))


# ---------------------------------------------------------------------------------------------------------------------
# the float64 references on three elements, by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_references_by_hand():
    x = torch.tensor([[1.0, -2.0, 3.0]])
    r = SC.logit_reference(Case(B=1, T=3, pos=1), REAL, dict(x=x, nf=torch.tensor([2])))['out'].tolist()
    assert r[0] == pytest.approx(2.0 / 3.0, rel=1e-15) and r[1] == pytest.approx(math.sqrt(114.0 / 27.0), rel=1e-15)
    assert r[2:] == [1.0, 2.0, 0.5]
    r = SC.logit_reference(Case(B=1, T=3, pos=0), REAL, dict(x=x, nf=torch.tensor([0])))['out'].tolist()
    assert r[2:4] == [0.0, 0.0] and math.isnan(r[4])          # 0 / 0 in fp32
    r = SC.vec_reference(Case(n=3, sign=-1.0), REAL, dict(v=torch.tensor([1.0, 2.0, 6.0])))['out'].tolist()
    assert r[0] == -3.0 and r[1] == pytest.approx(math.sqrt(14.0 / 3.0), rel=1e-15)
    r = SC.sqnorm_reference(Case(B=1, L=3, finish=1, commit=0), REAL, dict(x=torch.tensor([[1.0, 2.0, 3.0]]), nf=torch.tensor([2]), scale=25.0))
    assert r['part'].tolist() == [175.0] and r['out'].tolist() == [175.0]
    c = Case(cap=2, row=1, seq=4, cols='imm', pc=0, npart=3, calls=2)
    inp = dict(cols=[('imm', None)] * 2 + [('imm', 1.0), ('imm', -1)] + [('src', 'i', 9)] * 12, part=torch.tensor([1.0, 2.0, 6.0]))
    r = SC.commit_reference(c, REAL, inp)
    assert r['ring'].tolist() == [[0x40400000, 5, 0x3F800000, -1] + [9] * 12, [0x40400000, 4, 0x3F800000, -1] + [9] * 12]
    assert r['cursor'].tolist() == [1, 6]
    # one zero-padded frame of three samples: the DFT sum written out
    c = Case(B=1, L=3, lens=None)
    r = SC.ltas_reference(c, REAL, dict(x=torch.tensor([[1.0, 2.0, 3.0]])))
    w = [0.5 - 0.5 * math.cos(2.0 * math.pi * i / 256) for i in range(3)]
    f = [1.0 * w[0], 2.0 * w[1], 3.0 * w[2]]
    for k in (0, 1, 77, 128):
        re_ = sum(f[i] * math.cos(2.0 * math.pi * i * k / 256) for i in range(3))
        im_ = sum(f[i] * math.sin(2.0 * math.pi * i * k / 256) for i in range(3))
        assert float(r['out'][0, k]) == pytest.approx(re_ * re_ + im_ * im_, rel=1e-12)
    assert r['nframes'].tolist() == [1] and r['energy'][0] == pytest.approx(sum(v * v for v in f), rel=1e-15)
    c = Case(B=1, T=3, target=0.0, pos=1, calls=1)
    x = torch.tensor([[0.5, -1.0, float('nan')]])
    r = SC.score_reference(c, REAL, dict(x=x, nf=torch.tensor([2]), start=torch.zeros(6, dtype=torch.float64)))
    want = [1.0, (math.log1p(math.exp(0.5)) + math.log1p(math.exp(-1.0))) / 2.0, 2.0, 1.0, -0.5, 1.25]
    assert r['acc'].tolist() == pytest.approx(want, rel=1e-15)


def test_extremes_row_the_stable_form_and_float64_agree():
    """around the under- and overflow of expf the contract's fp32 form and float64 give the same loss, and float64 stays
    finite (checked before the row was pinned)"""
    x = torch.tensor([SC.EXTREMES])
    for tg in (0.0, 0.5, 0.9):
        c = Case(B=1, T=len(SC.EXTREMES), target=tg, pos=1, calls=1)
        ref = SC.score_reference(c, REAL, dict(x=x, nf=None, start=torch.zeros(6, dtype=torch.float64)))
        acc = EM.score_accum(x, None, tg, True, torch.zeros(6, dtype=torch.float64))
        assert np.isfinite(ref['add']).all() and bool(torch.isfinite(acc).all())
        assert abs(float(acc[1]) - ref['add'][1]) <= 16 * 2.0 ** -24 * ref['add'][1]


def test_plans_and_lists():
    for fam in SC.ORDER:
        F = SC.FAMILIES[fam]
        assert [l for l, _ in F.cases()] == [l for l, _ in F.cases()], fam
        assert len(set(l for l, _ in F.cases())) == len(F.cases()), ('labels are unique', fam)
        SC.picked(fam)
    assert (SC.COLS, SC.LT_BINS, SC.LT_CH) == (SM.COLS, EM.BINS, 16)
    assert [SC.lt_frames(L) for L in SC.LT_L] == [1, 1, 1, 1, 1, 1, 2, 3, 16, 17, 18, 33]
    assert [SC.lt_frames(L) for L in SC.LT_L] == [EM.frame_count(L) for L in SC.LT_L]
    # exact passes: |x| <= 3 over at most 2^22 entries: every partial sum of x and of x^2 is an integer below 2^53
    assert 9 * SC.LIMIT < 2 ** 53


DROPS = dict(logit=lambda l: '2048x2048' in l, vec=lambda l: l.startswith('n4097 '), sqnorm=lambda l: l.startswith('B65 L4 '),
             commit=lambda l: 'row5' in l, ltas=lambda l: l.startswith('L2304 '), score=lambda l: 'calls10' in l)


@pytest.mark.parametrize('fam', SC.ORDER)
def test_coverage_assertion_fails_when_a_class_is_not_reached(fam):
    F = SC.FAMILIES[fam]
    seen = [(l, c, F.plan(c)) for l, c in F.cases()]
    F.coverage(seen)
    with pytest.raises(AssertionError, match='never reached'):
        F.coverage([s for s in seen if not DROPS[fam](s[0])])


# ---------------------------------------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------------------------------------
class Mutant(SC.CpuModel):
    """one mistake per name; every other call is the model's"""

    def logit_summary(self, cls, nframes, positive, out=None):
        mut = self.mutate
        if not mut.startswith('logit_'):
            return SC.CpuModel.logit_summary(self, cls, nframes, positive, out)
        B, T = cls.shape
        x = cls.detach().double()
        n = nframes if nframes is not None else torch.full((B,), T, dtype=torch.long)
        ar = torch.arange(T).view(1, T)
        mask = (ar <= n.view(B, 1)) if mut == 'logit_mask_le' else (ar < n.view(B, 1))
        if mut == 'logit_hit_ge':
            hit = ((x >= 0) if positive else (x <= 0)) & mask
        else:
            hit = ((x > 0) if positive else (x < 0)) & mask
        mean = x[mask].mean() if mut == 'logit_mean_valid' and bool(mask.any()) else x.mean()
        if mut == 'logit_ddof1':
            std = (((x - mean) ** 2).sum() / (x.numel() - 1)).sqrt()
        elif mut == 'logit_onepass_f32':
            xf = cls.detach().float()
            std = ((xf * xf).mean() - xf.mean() ** 2).clamp(min=0).sqrt().double()
        else:
            std = ((x - mean) ** 2).mean().sqrt()
        h, c = hit.sum().float(), mask.sum().float()
        return out.copy_(torch.stack([mean.float(), std.float(), h, c, h / c]))

    def vec_stats(self, v, sign=1.0, out=None):
        SC.CpuModel.vec_stats(self, v, sign, out)
        if self.mutate == 'vec_sign_on_std':
            out[1] *= sign
        return out

    def sqnorm_rows(self, gx, nframes, scale, part=None, out=None, finish=True):
        B, L = gx.shape
        if self.mutate == 'sq_tail_dropped':
            n = nframes if nframes is not None else torch.full((B,), L, dtype=torch.int64)
            return SM.sqnorm_rows(gx[:, :L - L % 4], n, scale, part, out, finish)
        if self.mutate == 'sq_div_L':
            nframes = None
        return SM.sqnorm_rows(gx, nframes, scale, part, out, finish)

    def summary_commit(self, ring, cursor, cols, part=None, part_col=-1):
        mut = self.mutate
        row, cap = int(cursor[0]), ring.size(0)
        if mut == 'commit_bad_cursor_write' and not 0 <= row < cap:
            ring.as_strided((SC.COLS,), (1,), ring.storage_offset() + row * SC.COLS).fill_(1)      # (inside the frame's guard rows)
            return
        if mut == 'commit_imm_before_src':
            cols = [None if torch.is_tensor(c) else c for c in cols]           # the immediate (0) taken where src is set
        SC.CpuModel.summary_commit(self, ring, cursor, cols, part, part_col)
        if not 0 <= row < cap:
            return
        if mut == 'commit_src_before_seq' and torch.is_tensor(cols[1]):
            ring[row, 1] = cols[1].reshape(1).clone().view(torch.int32)[0]
        if mut == 'commit_no_wrap':
            cursor[0] = row + 1

    def _ltas(self, x, lens, out):
        mut = self.mutate
        B, L = x.shape
        S = SC.cdiv(SC.lt_frames(L), SC.LT_CH)
        for b in range(B):
            n = L if lens is None else max(0, min(int(lens[b]), L))
            if mut == 'lt_read_past_n' and n < SC.LT_N <= L:
                p = self.frame_powers(x[b], SC.LT_N)          # the read guard against L where n belongs
            else:
                p = self.frame_powers(x[b], n)
            nf = p.size(0)
            if mut == 'lt_odd_dropped':
                out[b] = p[0::2].sum(0) / nf
            if mut == 'lt_nyq_is_dc':
                out[b, 128] = out[b, 0]
            if mut == 'lt_div_S16':
                out[b] = p.sum(0) / (S * SC.LT_CH)
            if mut == 'lt_read_past_n':
                out[b] = p.sum(0) / nf

    def ltas_power(self, x, lens, out=None, nframes=None):
        EM.ltas_power(x, lens, out, nframes)
        self._ltas(x, lens, out)
        return out

    def ltas_raw(self, x, lens, out, nframes, slab):
        SC.CpuModel.ltas_raw(self, x, lens, out, nframes, slab)
        self._ltas(x, lens, out)
        if self.mutate == 'lt_finish_all_S':
            for b in range(x.size(0)):
                if bool(torch.isnan(slab[b]).any()):          # (a clip with every chunk: the same sum)
                    out[b] = slab[b].sum(0) / float(nframes[b])

    def score_accum(self, cls, nframes, target, positive, acc):
        mut = self.mutate
        B, T = cls.shape
        if mut == 'sc_rows16':
            cls, nframes, B = cls[:16], (nframes[:16] if nframes is not None else None), min(B, 16)
        add = EM.score_accum(cls, nframes, target, positive, torch.zeros(6, dtype=torch.float64))
        n = torch.full((B,), T, dtype=torch.int64) if nframes is None else nframes.clamp(0, T)
        if mut == 'sc_mean_over_T':
            one = torch.zeros(6, dtype=torch.float64)
            add[1] = 0.0
            for b in range(B):
                if int(n[b]) >= 1:
                    one.zero_()
                    EM.score_accum(cls[b:b + 1], n[b:b + 1], target, positive, one)
                    add[1] += one[1] * int(n[b]) / T
        if mut == 'sc_empty_counted':
            add[0] = B
        if mut == 'sc_overwrite':
            return acc.copy_(add)
        acc += add
        return acc


WORD, OOB, BITS, NANOUT, OUTSIDE = ('word differs|more than one unit in the last place', 'real pass: out of bound',
                                    'differs in its bits', 'NaN or infinity in the output', 'wrote outside its window')
# (what is mutated, family, the assertion that has to fire, the output it has to fire on)
MUTANTS = [
    ('logit_mask_le', 'logit', WORD, '(hits|mask)'),              # the mask taken with <= where < belongs
    ('logit_mean_valid', 'logit', WORD, 'mean'),                  # the mean over the valid entries only
    ('logit_ddof1', 'logit', WORD, 'std'),                        # the sample variance
    ('logit_onepass_f32', 'logit', WORD, 'std'),                  # E[x^2] - m^2 in fp32
    ('logit_hit_ge', 'logit', WORD, 'hits'),                      # a zero counted as a hit
    ('vec_sign_on_std', 'vec', WORD, 'std'),                      # the sign applied to the std as well
    ('sq_tail_dropped', 'sqnorm', OOB, '(commit|out|part)'),      # the L % 4 elements behind the last whole quad dropped
    ('sq_div_L', 'sqnorm', OOB, '(commit|out|part)'),             # divided by L when nframes is given
    ('commit_src_before_seq', 'commit', BITS, 'ring'),            # column 1 from src where the sequence number belongs
    ('commit_imm_before_src', 'commit', BITS, 'ring'),            # the immediate taken where src is set
    ('commit_no_wrap', 'commit', BITS, '(ring|cursor)'),          # the cursor not wrapped at capacity
    ('commit_bad_cursor_write', 'commit', OUTSIDE, 'ring'),       # a row written through a cursor out of range
    ('lt_odd_dropped', 'ltas', OOB, 'out'),                       # the odd frame of every pair dropped
    ('lt_nyq_is_dc', 'ltas', OOB, 'out'),                         # bin 128 read from the slot of bin 0
    ('lt_div_S16', 'ltas', OOB, 'out'),                           # divided by S * 16 frames
    ('lt_finish_all_S', 'ltas', NANOUT, 'out'),                   # the finishing launch adds all S chunks
    ('lt_read_past_n', 'ltas', NANOUT, 'out'),                    # a frame read past n
    ('sc_mean_over_T', 'score', OOB, 'loss'),                     # the per-clip mean over T
    ('sc_empty_counted', 'score', WORD, 'clips'),                 # empty clips counted in word 0
    ('sc_overwrite', 'score', WORD, 'clips'),                     # acc overwritten where it is added to
    ('sc_rows16', 'score', WORD, 'clips'),                        # rows >= 16 dropped
]


@pytest.mark.parametrize('mutate,fam,what,output', MUTANTS)
def test_checker_rejects_a_mutant(mutate, fam, what, output):
    """the first assertion to fire is the one meant for the mutant, on the output it corrupts"""
    with pytest.raises(AssertionError, match="(%s).*\\('%s', '[^']*', '%s'\\)" % (what, fam, output)):
        SC.sweep(fam, Mutant(mutate=mutate), 'cpu')


def test_the_listed_mutants_cover_the_issue():
    assert len(MUTANTS) == 21 and len(set(m[0] for m in MUTANTS)) == 21
    assert all(re.match('(logit|vec|sq|commit|lt|sc)_', m[0]) for m in MUTANTS)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: host code, before any HIP call
# ---------------------------------------------------------------------------------------------------------------------
_HOST = ctypes.create_string_buffer(4096)
PTR = (ctypes.addressof(_HOST) + 15) & ~15


def test_launchers_refuse_before_any_hip_call():
    """AG_ERR_ARG from host code, with no device in sight (the pointers are host memory: a launch would not survive them)"""
    import audiogan_amd.kernels as K
    from audiogan_amd import _lib
    lib, bad = K.lib, _lib.AG_ERR_ARG
    p = ctypes.c_void_p(PTR)
    n = (1 << 22) + 1
    for B, T in ((1, n), (n, 1), (2049, 2048), (0, 4), (4, 0)):
        assert lib.ag_logit_summary(p, T, 1, p, 1, p, B, T, None) == bad, (B, T)
        assert lib.ag_score_accum(p, T, 1, p, 0.5, 1, p, B, T, None) == bad, (B, T)
    assert lib.ag_logit_summary(None, 4, 1, p, 1, p, 4, 4, None) == bad and lib.ag_logit_summary(p, 4, 1, p, 1, None, 4, 4, None) == bad
    assert lib.ag_score_accum(p, 4, 1, p, 0.5, 1, ctypes.c_void_p(PTR + 4), 4, 4, None) == bad           # acc displaced by 4 bytes
    assert b'ag_score_accum' in lib.ag_last_error()
    assert lib.ag_score_accum(p, 4, 1, p, 0.5, 1, None, 4, 4, None) == bad
    assert lib.ag_sqnorm_rows(p, 8, p, 1.0, p, p, 65536, 8, None) == bad
    assert lib.ag_sqnorm_rows(p, 7, p, 1.0, p, p, 4, 8, None) == bad                                     # ld < L
    assert lib.ag_sqnorm_rows(p, 8, p, 1.0, None, p, 4, 8, None) == bad
    assert lib.ag_vec_stats(p, 1.0, p, 0, None) == bad and lib.ag_vec_stats(p, 1.0, None, 4, None) == bad
    assert lib.ag_summary_commit(None, None) == bad
    # ag_ltas_power: L = 2304 has 17 frames, two chunks
    B, L = 2, 2304
    need = int(lib.ag_ltas_ws_numel(B, L))
    assert need == B * 2 * 129 and lib.ag_ltas_ws_numel(B, 2176) == 0 and lib.ag_ltas_ws_numel(0, L) == 0
    assert lib.ag_bind_workspace(None, 0) == 0
    assert lib.ag_ltas_power(p, L - 1, p, p, p, B, L, None) == bad                                      # ldx < L
    assert lib.ag_ltas_power(p, 255, p, p, p, B, 256, None) == bad
    assert lib.ag_ltas_power(p, L, p, p, p, B, L, None) == bad and b'bind a workspace' in lib.ag_last_error()      # none bound, S > 1
    assert lib.ag_bind_workspace(p, need - 1) == 0
    assert lib.ag_ltas_power(p, L, p, p, p, B, L, None) == bad and b'bind a workspace' in lib.ag_last_error()      # one float too small
    # a binding is taken by the call it was made for, refused or not: the next call does not see a stale one
    assert lib.ag_bind_workspace(p, need) == 0
    assert lib.ag_ltas_power(p, L - 1, p, p, p, B, L, None) == bad and b'bad args' in lib.ag_last_error()
    assert lib.ag_ltas_power(p, L, p, p, p, B, L, None) == bad and b'bind a workspace' in lib.ag_last_error()
    assert lib.ag_bind_workspace(None, 0) == 0
